"""Adaptive projected guidance without a device: both entries in the header, in EXPORTS and in the built library, their argument checks,
the wrapper's refusals, the host executor against the float32 restatement of the definition, and an untouched wrapper's route."""

import ctypes
import os

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, graphs, rolling
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
NAMES = ("skr_projected_guidance_coef", "skr_projected_guided_step_launch")


# ---- the definition restated: float32 torch ops for d and p, float64 for the coefficients (CPU tensors, dim 0 the sample) ----------------
def restate_d(u, c, m, beta):
    d = c.float() - u.float()
    if beta != 0.0:
        d = d + torch.tensor(beta, dtype=torch.float32) * m.float()
    return d.to(u.dtype)


def coefficients64(d, c, g, eta, r):
    "(A, B, sums) per sample in float64 over the T-valued d and c; sums = (Sdd, Sdc, Scc, sum |d c|)"
    dd, cd = d.double().reshape(d.shape[0], -1), c.double().reshape(c.shape[0], -1)
    sdd, sdc, scc = (dd * dd).sum(1), (dd * cd).sum(1), (cd * cd).sum(1)
    norm = sdd.sqrt()
    clamp = torch.where(norm > r, r / norm, torch.ones_like(norm)) if r > 0.0 else torch.ones_like(norm)
    root = scc.sqrt().clamp_min(1e-12)
    a = (g - 1.0) * clamp
    return a, 1.0 - a * (1.0 - eta) * (sdc / (root * root)), (sdd, sdc, scc, (dd * cd).abs().sum(1))


def restate_p(c, d, a32, b32):
    per_sample = (c.shape[0],) + (1,) * (c.ndim - 1)
    return (b32.reshape(per_sample) * c.float() + a32.reshape(per_sample) * d.float()).to(c.dtype)


def test_entries_are_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    lib = _hip.load()
    for name in NAMES:
        assert f"int {name}(" in header and name in _hip.EXPORTS and getattr(lib, name) is not None
    assert "#define SKR_PROJECTED_PARTIALS(" in header and _hip.projected_partials(3 * 2056, 2056) == 24


def aligned_buffer():
    buf = (ctypes.c_char * 128)()
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16


COEF_CASES = [  # (changed arguments, code): each case also breaks something checked later, so the order shows
    ({"uncond": None, "numel": -1}, NULL), ({"coef": None, "sn": 0}, NULL), ({"partials": None}, NULL), ({"mom": None, "sn": 0}, NULL),
    ({"numel": -8, "cond": 8}, SHAPE), ({"sn": 1}, SHAPE), ({"numel": 12}, SHAPE),
    ({"numel": 0, "cond": 8, "dtype": 99}, OK),
    ({"cond": 8, "dtype": 99}, ALIGN), ({"mom": 8, "dtype": 99}, ALIGN), ({"coef": 2, "dtype": 99}, ALIGN),
    ({"dtype": _hip.F64}, DTYPE), ({"dtype": 99}, DTYPE),
]  # fmt: skip


@pytest.mark.parametrize("changes,code", COEF_CASES)
def test_coef_entry_checks_in_their_documented_order(changes, code):
    "a pointer given as an int is the aligned buffer plus that offset; None is NULL; no launch is reached, so no memory is touched"
    _, good = aligned_buffer()
    a = {"uncond": 0, "cond": 0, "mom": 0, "dtype": _hip.BF16, "numel": 16, "sn": 8, "coef": 0, "partials": 0, **changes}
    ptr = lambda k: None if a[k] is None else good + a[k]  # noqa: E731
    status = _hip.load().skr_projected_guidance_coef(ptr("uncond"), ptr("cond"), ptr("mom"), a["dtype"], 7.5, 0.0, 2.0, -0.5, a["numel"], a["sn"], ptr("coef"), None,
                                                     ptr("partials"), None)  # fmt: skip
    assert status == code


STEP_CASES = [  # (changed fields: plan's, proj_..., guide_..., or the call's numel / out / inputs / proj, code)
    ({"proj": None}, NULL), ({"noise_mode": 1, "zeta0": 0.5, "n_terms": 99}, NULL),
    ({"n_terms": 17, "numel": -1}, TERMS), ({"guide_slot": 2, "numel": -1}, TERMS),
    ({"numel": -1, "noise_mode": 3}, SHAPE),
    ({"out0_dtype": _hip.NONE, "guide_guided_out": None, "noise_mode": 3}, NULL),
    ({"noise_mode": 3, "proj_sample_numel": 0}, UNSUPPORTED), ({"proj_reserved": 1, "proj_sample_numel": 0}, UNSUPPORTED),
    ({"guide_reserved": 1, "proj_sample_numel": 0}, UNSUPPORTED), ({"acc_f64": 1, "proj_sample_numel": 0}, UNSUPPORTED),
    ({"out0_dtype": _hip.NONE, "proj_sample_numel": 0}, UNSUPPORTED),
    ({"proj_sample_numel": 5, "guide_cond": None}, SHAPE), ({"proj_sample_numel": 1, "guide_cond": None}, SHAPE),
    ({"numel": 0, "inputs": None, "out": None, "guide_cond": None}, OK),
    ({"guide_cond": None, "out": 8}, NULL), ({"proj_coef_dev": None, "out": 8}, NULL), ({"inputs": None}, NULL),
    ({"guide_cond": 8, "dtype_a": 99}, ALIGN), ({"proj_diff": 8, "dtype_a": 99}, ALIGN), ({"proj_coef_dev": 2, "dtype_a": 99}, ALIGN),
    ({"dtype_a": _hip.F64, "dtype_b": _hip.F64, "out0_dtype": _hip.F64}, DTYPE), ({"dtype_a": 99}, DTYPE),
]  # fmt: skip


@pytest.mark.parametrize("changes,code", STEP_CASES)
def test_step_entry_checks_in_their_documented_order(changes, code):
    _, good = aligned_buffer()
    at = lambda v: None if v is None else good + v  # noqa: E731
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    proj = _hip.StepProjectionC(good, None, 8, 0)
    guide = _hip.StepGuidanceC(good, good, 0.0, 0, 0)
    call = {"numel": 16, "out": 0, "inputs": (ctypes.c_void_p * 2)(good, good), "proj": proj}
    for k, v in changes.items():
        if k in call:
            call[k] = v
        elif k.startswith(("proj_", "guide_")):
            target, field = (proj, k[5:]) if k.startswith("proj_") else (guide, k[6:])
            setattr(target, field, at(v) if field in ("coef_dev", "diff", "cond", "guided_out") else v)
        else:
            setattr(plan, k, v)
    status = _hip.load().skr_projected_guided_step_launch(ctypes.byref(plan), call["inputs"], at(call["out"]), ctypes.byref(guide),
                                                          ctypes.byref(proj) if call["proj"] is not None else None, None, call["numel"], None)  # fmt: skip
    assert status == code


def wrapper(sampler=None, **projection):
    w = PD.SkrampleWrapperScheduler(sampler or PT.DPM(order=2), PS.Karras(PS.Scaled()))
    if projection:
        w.set_projected_guidance(**projection)
    w.set_timesteps(4)
    return w


def test_refusals_name_their_reason():
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(0))
    w = wrapper(eta=0.0, norm_threshold=2.0, momentum=-0.5)
    t = w.timesteps[0]
    with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale"):
        w.step_guided(x, x + 1, 5.0, t, x, guidance_rescale=0.7)
    with pytest.raises(_hip.SkrampleHipError, match="fp64"):
        w.step_guided(x.double(), x.double() + 1, 5.0, t, x.double())
    with pytest.raises(_hip.SkrampleHipError, match="autograd"):
        w.step_guided(x.clone().requires_grad_(), x + 1, 5.0, t, x)
    with pytest.raises(_hip.SkrampleHipError, match="in-painting"):
        w.set_inpaint(torch.ones(8, 8), x, x)
    with pytest.raises(_hip.SkrampleHipError, match="thresholding"):
        w.set_thresholding(0.9, 1.5)
    for setter in (lambda v: v.set_inpaint(torch.ones(8, 8), x, x), lambda v: v.set_thresholding(0.9, 1.5)):  # ... and in the other order
        v = wrapper()
        setter(v)
        with pytest.raises(_hip.SkrampleHipError, match="set_projected_guidance"):
            v.set_projected_guidance(0.0)
    with pytest.raises(_hip.SkrampleHipError, match="no row form"):
        graphs.capture_sampling_loop(w, lambda s, t: (s, s), x, 4)
    with pytest.raises(_hip.SkrampleHipError, match="no row form"):
        rolling.RollingBatch(lambda: w, torch.zeros(2, 4, 32, 16, dtype=torch.bfloat16), capacity=2)
    assert not hasattr(PD.RKWrapperCore, "set_projected_guidance")


@pytest.mark.parametrize("sampler", [PT.DPM(order=2), PT.UniPC(order=2)], ids=lambda s: type(s).__name__)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_host_executor_is_the_float32_restatement(sampler, dtype):
    "4 steps on CPU tensors: prev_sample against a twin wrapper's step() over the restated p, the running average against the restated d"
    g, shape, (scale, eta, r, beta) = torch.Generator().manual_seed(3), (3, 3, 8, 8), (7.5, 0.0, 4.0, -0.5)
    w, twin = wrapper(sampler, eta=eta, norm_threshold=r, momentum=beta), wrapper(sampler)
    x, m = (torch.randn(shape, generator=g) * float(w.init_noise_sigma)).to(dtype), torch.zeros(shape, dtype=dtype)
    for t in w.timesteps:
        u, c = (torch.randn(shape, generator=g).to(dtype) for _ in range(2))
        d = restate_d(u, c, m, beta)
        a, b, (sdd, *_) = coefficients64(d, c, scale, eta, r)
        assert (sdd.sqrt() > r).any()  # the clamp is in play
        got = w.step_guided(u, c, scale, t, x, return_dict=False)[0]
        ref = twin.step(restate_p(c, d, a.float(), b.float()), t, x, return_dict=False)[0]
        assert torch.equal(got, ref) and torch.equal(w._projection.momentum_buf, d)
        x, m = got, d
    w.set_timesteps(4)
    assert not w._projection.momentum_buf.any()


def test_untouched_wrapper_never_reaches_the_new_launches(monkeypatch):
    calls = []
    monkeypatch.setattr(_hip, "launch_projected_coef", lambda *a, **k: calls.append("coef"))
    monkeypatch.setattr(_hip, "launch_projected_guided_step", lambda *a, **k: calls.append("step"))
    x = torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(1))
    for w in (wrapper(), wrapper(eta=None)):
        _hip.trace = []
        try:
            w.step_guided(x, x + 1, 5.0, w.timesteps[0], x)
            assert not calls and not any(getattr(call, "kind", None) == "guided_projected" for call in _hip.trace)
        finally:
            _hip.trace = None
        assert getattr(w, "_projection", None) is None
