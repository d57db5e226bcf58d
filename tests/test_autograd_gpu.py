"""Autograd through the device steps (lazy._StepFunction / native._TapeFunction / lazy._PowerBlendFunction and the kernels behind them,
csrc/skr_step_backward.hip and skr_power_blend_backward).  The yardstick is the package's own host executor on float64 CPU copies, which
is differentiable by construction, and torch.autograd.gradcheck on float64 device tensors."""

import ctypes

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.common import DeltaPoint, Point, Step
from skrample_amd.sampling import lazy, native
from skrample_amd.sampling import models as PM
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPE = (2, 4, 8, 8)


def _net(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Conv2d(4, 4, 3, padding=1)
    with torch.no_grad():
        net.weight.mul_(0.3)
    return net


WRAPPERS = {
    "dpm2": lambda **kw: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()), **kw),
    "euler": lambda **kw: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled(), **kw),
    "adams4": lambda **kw: PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.Scaled(), **kw),
    "unipc3": lambda **kw: PD.SkrampleWrapperScheduler(PT.UniPC(order=3), PS.Karras(PS.Scaled()), **kw),
    "rkultra": lambda **kw: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=3, **kw),
}


def _loop(make, x, net, steps=5, static=False, **kw):
    w = make(**kw)
    w.set_timesteps(steps)
    buf = torch.empty_like(x) if static else None
    for t in w.timesteps:
        out = net(x)
        if static:  # a network that writes into one buffer (torch.compile "reduce-overhead" style)
            buf.copy_(out)
            out = buf
        x = w.step(out, t, x, return_dict=False)[0]
    return x


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_wrapper_loop_gradients_match_the_host_run(name):
    "device fp32 latents that require grad: the result has a grad_fn, and latent / weight gradients match the float64 CPU run to 1e-5"
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(SHAPE, generator=g, dtype=torch.float64)
    target = torch.randn(SHAPE, generator=g, dtype=torch.float64)
    net_h = _net().double()
    net_d = _net().to(DEV)
    xh = x0.clone().requires_grad_()
    xd = x0.float().to(DEV).requires_grad_()
    out_h = _loop(WRAPPERS[name], xh, net_h)
    out_d = _loop(WRAPPERS[name], xd, net_d)
    assert out_d.grad_fn is not None and out_d.is_cuda
    ((out_h - target) ** 2).mean().backward()
    ((out_d - target.float().to(DEV)) ** 2).mean().backward()
    assert xd.grad is not None and net_d.weight.grad is not None
    assert _rel(xd.grad, xh.grad) < 1e-5, name
    assert _rel(net_d.weight.grad, net_h.weight.grad) < 1e-5, name
    assert _rel(net_d.bias.grad, net_h.bias.grad) < 1e-5, name


def _dev64(*shape, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) + shift).to(DEV).requires_grad_()


SAMPLERS = {
    "euler_sde": lambda: PT.Euler(stochasticity=1),
    "dpm1": lambda: PT.DPM(order=1),
    "dpm3_sde": lambda: PT.DPM(order=3, stochasticity=0.5),
    "adams4": lambda: PT.Adams(order=4),
    "unip3": lambda: PT.UniP(order=3),
    "unipc3_sde": lambda: PT.UniPC(order=3, stochasticity=1),
    "spc": lambda: PT.SPC(),
    "spc_power2": lambda: PT.SPC(power=2),
}


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_gradcheck_sampler_steps(name):
    "three steps of each family on float64 device tensors; SDE steps take a fixed noise tensor; UniPC returns both outputs"
    sampler, model, sched = SAMPLERS[name](), PM.NoiseModel(), PS.Scaled()
    shift = 4.0 if "power" in name else 0.0  # the signed-power blend: operands away from 0
    xs = _dev64(1, 2, 8, seed=3, shift=shift)
    outs = [_dev64(1, 2, 8, seed=10 + i) * 0.1 for i in range(3)]
    noise = [torch.randn(1, 2, 8, dtype=torch.float64).to(DEV) for _ in range(3)]

    def f(x, o0, o1, o2):
        previous = []
        res = []
        for i, o in enumerate((o0, o1, o2)):
            rec = sampler.sample(x, o, Step.from_int(i + 2, 8), model, sched, noise[i] if sampler.require_noise else None, tuple(previous))
            previous.append(rec)
            x = rec.final
            res.append(rec.final)
            if type(sampler) is PT.UniPC:
                res.append(rec.sample)
        return tuple(res)

    assert torch.autograd.gradcheck(f, (xs, *[o.detach().requires_grad_() for o in outs]), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradcheck_wrapper_sde_steps_with_in_kernel_philox():
    "a DPM-2 SDE wrapper step draws its noise inside the kernel; seeded generators make it deterministic, so gradcheck applies"
    x, o = _dev64(2, 1, 8, 8, seed=4), _dev64(2, 1, 8, 8, seed=5)

    def f(x, o):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), compute_scale=torch.float64)
        w.set_timesteps(4)
        gens = [torch.Generator().manual_seed(s) for s in (11, 12)]
        y = w.step(o, w.timesteps[0], x, generator=gens, return_dict=False)[0]
        return w.step(o * 0.5, w.timesteps[1], y, generator=gens, return_dict=False)[0]

    assert torch.autograd.gradcheck(f, (x, o), eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("kinds", [(t, f) for t in range(4) for f in range(4) if (t, f) != (0, 0)])  # ((0, 0) is no conversion)
def test_gradcheck_rounded_conversion_stage(kinds):
    to_kind, from_kind = kinds
    k = [0.83, 1.7, 0.41, 2.3]
    s, o, extra = _dev64(2, 64, seed=1), _dev64(2, 64, seed=2), _dev64(2, 64, seed=3)

    def f(s, o, extra):
        conv = lazy.RoundedConversion(s, o, to_kind, from_kind, k)
        form = conv.node() * 0.7 + lazy.Lin.leaf(s) * 0.2 + lazy.Lin.leaf(extra) * -1.1
        return tuple(lazy.evaluate([conv, form], [None, torch.float64]))

    assert torch.autograd.gradcheck(f, (s, o, extra), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradcheck_noise_functions_and_model_transforms():
    x, n = _dev64(2, 4, 4, 4, seed=6), _dev64(2, 4, 4, 4, seed=7)
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()), compute_scale=torch.float64)
    w.set_timesteps(6)
    t = w.timesteps[2]
    pt = Point(613.0, 0.7391, 0.6733)
    v = PM.VelocityModel()
    checks = [
        lambda x, n: w.add_noise(x, n, w.timesteps[2:3]),
        lambda x, n: w.scale_noise(x, t, n),
        lambda x, n: pt.add_noise(x, n),
        lambda x, n: pt.remove_noise(x, n),
        lambda x, n: v.to_x(x, n, pt),
        lambda x, n: v.from_x(x, n, pt),
        lambda x, n: v.forward(x, n, DeltaPoint(pt, Point(500.0, 0.5, 0.86))),
    ]
    for fn in checks:
        assert torch.autograd.gradcheck(fn, (x, n), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradcheck_power_blend_and_zero_semantics():
    a, b = _dev64(3, 64, seed=8, shift=3.0), _dev64(3, 64, seed=9, shift=-3.0)
    for power in (2.0, 0.5, 3.0):
        assert torch.autograd.gradcheck(lambda a, b: lazy.power_blend(a, b, 0.6, 0.4, power, torch.float64), (a, b), eps=1e-7, atol=1e-6, rtol=1e-5)
    # exact zeros: what torch autograd of the host expression gives (0 where the exponent is >= 0, NaN where 0 meets a negative power)
    for power in (2.0, 0.5):
        av = torch.tensor([0.0, 1.5, 0.0, -2.0], dtype=torch.float64)
        bv = torch.tensor([0.0, 0.0, 2.0, 2.0], dtype=torch.float64)
        ah, bh = av.clone().requires_grad_(), bv.clone().requires_grad_()
        lazy.power_blend(ah, bh, 0.5, 0.5, power, torch.float64).sum().backward()
        ad, bd = av.to(DEV).requires_grad_(), bv.to(DEV).requires_grad_()
        lazy.power_blend(ad, bd, 0.5, 0.5, power, torch.float64).sum().backward()
        for got, want in ((ad.grad, ah.grad), (bd.grad, bh.grad)):
            got = got.cpu()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (power, got, want)
            torch.testing.assert_close(torch.nan_to_num(got), torch.nan_to_num(want), rtol=1e-12, atol=1e-12)


ALIAS = [True, False, "auto"]


@pytest.mark.parametrize("setting", [("fp32", torch.float32, torch.float32), ("bf16", torch.bfloat16, torch.float32), ("tape", torch.bfloat16, None)])
def test_forward_bits_are_unchanged_under_grad(setting):
    _, dtype, scale = setting
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(SHAPE, generator=g).to(dtype).to(DEV)
    make = WRAPPERS["adams4"]
    grads = []
    for static in (False, True):
        for alias in ALIAS:
            if static and alias is True:
                continue  # (aliasing a reused buffer is refused by the wrapper's guard, with or without grad)
            net = _net().to(DEV).to(dtype)
            with torch.no_grad():
                plain = _loop(make, x0, net, static=static, alias_history=alias, compute_scale=scale)
            x = x0.clone().requires_grad_()
            got = _loop(make, x, net, static=static, alias_history=alias, compute_scale=scale)
            assert got.grad_fn is not None and got.dtype == plain.dtype
            assert torch.equal(got.detach(), plain), (setting, static, alias)
            got.float().square().mean().backward()
            grads.append((x.grad.clone(), net.weight.grad.clone()))
    for gx, gw in grads[1:]:
        assert torch.equal(gx, grads[0][0]) and torch.equal(gw, grads[0][1])


def test_no_grad_no_change(monkeypatch):
    "without tensors that require grad no autograd Function is made and the replayed-step path serves the steps as before"
    def refuse(*a, **k):
        raise AssertionError("autograd Function used without requires_grad")

    monkeypatch.setattr(lazy._StepFunction, "apply", refuse)
    monkeypatch.setattr(native._TapeFunction, "apply", refuse)
    monkeypatch.setattr(lazy._PowerBlendFunction, "apply", refuse)
    x0 = torch.randn(SHAPE, device=DEV)
    w = WRAPPERS["dpm2"]()
    for _run in range(3):  # (the replayed-step path serves in-order runs from the second one on)
        w.set_timesteps(8)
        x = x0
        for t in w.timesteps.tolist():
            x = w.step(x * 0.5, t, x, return_dict=False)[0]
    assert x.grad_fn is None
    assert w._fast_hits > 0
    monkeypatch.undo()
    hits = w._fast_hits
    w.set_timesteps(8)  # the same wrapper under grad: the general path, never the replayed one
    x = x0.clone().requires_grad_()
    for t in w.timesteps.tolist():
        x = w.step(x * 0.5, t, x, return_dict=False)[0]
    assert x.grad_fn is not None and w._fast_hits == hits
    y = PT.SPC(power=2).sample(x0, x0 * 0.1, Step.from_int(2, 8), PM.NoiseModel(), PS.Scaled(), None, ())
    assert y.final.grad_fn is None


def test_linear_run_saves_no_tensors_and_the_blend_saves_two():
    saved = []

    def pack(t):
        saved.append(t.shape)
        return t

    x = torch.randn(SHAPE, device=DEV).requires_grad_()
    w = WRAPPERS["dpm2"]()
    w.set_timesteps(20)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = x
        for t in w.timesteps:
            y = w.step(-y, t, y, return_dict=False)[0]
    assert y.grad_fn is not None and saved == []
    y.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    a, b = (torch.randn(SHAPE, device=DEV) + 3).requires_grad_(), (torch.randn(SHAPE, device=DEV) + 3).requires_grad_()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        lazy.power_blend(a, b, 0.5, 0.5, 2.0)
    assert len(saved) == 2


def test_nonlinear_tape_under_grad_is_refused():
    a = torch.randn(2, 4, 64, device=DEV, dtype=torch.bfloat16).requires_grad_()
    b = torch.randn(2, 4, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(_hip.SkrampleHipError, match="MUL"):
        native._express(a, lambda p, q: p * q, a, b)
    with torch.no_grad():  # (without grad the same tape runs)
        assert torch.equal(native._express(a, lambda p, q: p * q, a, b), a.detach() * b)


# ---- the C ABI directly ------------------------------------------------------------------------------------------------------------------
def _ulp(t: torch.Tensor, dtype) -> torch.Tensor:
    "unit in the last place of |t| in `dtype`, subnormals included"
    info = torch.finfo(dtype)
    mant = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23, torch.float64: 52}[dtype]
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(info.tiny))) - mant)


def _abi_case(k, dtypes, g_dtype, has1, numel, acc_f64, seed):
    g = torch.Generator().manual_seed(seed)
    g0 = torch.randn(numel, generator=g).to(g_dtype).to(DEV)
    g1 = torch.randn(numel, generator=g).to(g_dtype).to(DEV) if has1 else None
    a = [float(v) for v in torch.randn(k, generator=g, dtype=torch.float64)]
    b = [float(v) for v in torch.randn(k, generator=g, dtype=torch.float64)]
    like = [lazy._Like((numel,), dtypes[0] if j < (k + 1) // 2 else dtypes[1]) for j in range(k)]
    return g0, g1, a, b, like


@pytest.mark.parametrize("numel", [8 * 2048, 4 * 1024 + 5])
@pytest.mark.parametrize("has1", [False, True])
@pytest.mark.parametrize("group", [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16), (torch.float32, torch.float32), (torch.float64, torch.float64), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16, 17, 80])
def test_backward_kernel_abi(k, group, has1, numel):
    lib = _hip.load()
    acc_f64 = group[0] == torch.float64
    g_dtype = group[0]
    g0, g1, a, b, like = _abi_case(k, group, g_dtype, has1, numel, acc_f64, seed=k * 7 + numel)
    try:
        fast = lazy.launch_backward(g0, g1, a, b, like, acc_f64)
        lib.skr_set_tuning(b"one_trip", 0)
        general = lazy.launch_backward(g0, g1, a, b, like, acc_f64)
    finally:
        lib.skr_set_tuning(b"reset", 0)
    torch.cuda.synchronize()
    x0, x1 = g0.double().cpu(), (g1.double().cpu() if has1 else None)
    for j in range(k):
        assert torch.equal(fast[j], general[j]), (k, group, has1, numel, j)
        assert fast[j].dtype == like[j].dtype and fast[j].shape == like[j].shape
        ca, cb = (a[j], b[j]) if acc_f64 else (float(torch.tensor(a[j], dtype=torch.float32)), float(torch.tensor(b[j], dtype=torch.float32)))
        exact = ca * x0 + (cb * x1 if has1 else 0.0)
        want = exact.to(like[j].dtype)
        got = fast[j].cpu()
        if not has1:  # one product: its correctly rounded value, rounded once more to the gradient dtype at most
            assert ((got.double() - want.double()).abs() <= _ulp(want.double(), like[j].dtype) * (0 if acc_f64 else 1)).all(), (k, group, j)
        else:  # fma(b, g1, a*g0) in the register type, then one rounding: the product's rounding bounds the difference
            eps = 2.0**-53 if acc_f64 else 2.0**-24
            bound = _ulp(torch.maximum(want.double().abs(), got.double().abs()), like[j].dtype) + 2 * eps * (abs(ca) * x0.abs() + abs(cb) * x1.abs())
            assert ((got.double() - exact).abs() <= bound).all(), (k, group, j)


def test_backward_kernel_refuses_bad_plans():
    lib = _hip.load()
    plan = _hip.StepGradPlanC()
    plan.n_grads = 0
    assert lib.skr_step_backward_launch(ctypes.byref(plan), None, None, None, 16, None) == 3
    plan.n_grads, plan.n_group_a, plan.dtype_a, plan.g0_dtype, plan.g1_dtype = 1, 1, _hip.F32, _hip.F32, _hip.NONE
    out = torch.empty(32, device=DEV)
    arr = (ctypes.c_void_p * 1)(out.data_ptr())
    assert lib.skr_step_backward_launch(ctypes.byref(plan), None, None, arr, 16, None) == 1
    assert lib.skr_step_backward_launch(ctypes.byref(plan), out.data_ptr() + 4, None, arr, 16, None) == 4
    plan.g0_dtype = 9
    assert lib.skr_step_backward_launch(ctypes.byref(plan), out.data_ptr(), None, arr, 16, None) == 2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_backward_kernel_abi_f64_arithmetic_into_16bit_gradients(dtype):
    "acc_f64 with 16-bit gradients: fp64 registers, then fp64 -> fp32 -> dtype as the forward's stores round (grid-stride kernel)"
    for k, numel in ((3, 8 * 2048), (17, 4 * 1024 + 5)):
        g0, g1, a, b, like = _abi_case(k, (dtype, dtype), torch.float32, True, numel, True, seed=k + numel)
        got = lazy.launch_backward(g0, g1, a, b, like, True)
        x0, x1 = g0.double().cpu(), g1.double().cpu()
        for j in range(k):
            exact = a[j] * x0 + b[j] * x1
            want = exact.float().to(dtype)
            err = (got[j].cpu().double() - want.double()).abs()
            assert (err <= _ulp(want.double(), dtype)).all() and (err == 0).float().mean() > 0.99, (dtype, k, j)


def _tape_steps(sampler, xs, outs, steps=8):
    "three sampler-level steps on the given tensors (previous records carried), returning every tensor of every record"
    model, sched = PM.NoiseModel(), PS.Scaled()
    previous, res, x = [], [], xs
    for i, o in enumerate(outs):
        rec = sampler.sample(x, o, Step.from_int(i + 2, steps), model, sched, None, tuple(previous))
        previous.append(rec)
        keep = sampler.require_previous
        previous = previous[max(len(previous) - keep, 0) :] if keep else []
        x = rec.final
        res += [t for t in (rec.final, rec.sample, torch.as_tensor(rec.prediction)) if isinstance(t, torch.Tensor) and t.requires_grad]
    return res


@pytest.mark.parametrize("name", ["dpm2", "adams3", "unipc3_deriv", "unip2"])
def test_tape_gradients_match_autograd_of_the_host_tape(name, monkeypatch):
    """op-tape steps (compute_scale=None, here fp32 with native.mode = "always") on device tensors that require grad: the gradients of the
    folded tape equal torch autograd of the same tapes run op by op on float64 CPU copies (UniPC stores up to three values: the pairwise
    sum of the backward launches)"""
    sampler = {"dpm2": PT.DPM(order=2), "adams3": PT.Adams(order=3), "unipc3_deriv": PT.UniPC(order=3, derivative_transform=PM.VelocityModel()),
               "unip2": PT.UniP(order=2)}[name]  # fmt: skip
    monkeypatch.setattr(native, "mode", "always")
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64)
    o0 = [torch.randn(2, 4, 8, 8, generator=g, dtype=torch.float64) * 0.3 for _ in range(3)]
    leaves_h = [x0.clone().requires_grad_(), *[o.clone().requires_grad_() for o in o0]]
    leaves_d = [t.detach().float().to(DEV).requires_grad_() for t in leaves_h]
    before = native.launches
    res_d = _tape_steps(sampler, leaves_d[0], leaves_d[1:])
    assert native.launches > before, "the steps did not take the op tape"
    res_h = _tape_steps(sampler, leaves_h[0], leaves_h[1:])
    assert len(res_d) == len(res_h) and all(r.grad_fn is not None for r in res_d if not r.is_leaf)  # (a record's sample may be the caller's leaf)
    assert sum(r.grad_fn is not None for r in res_d) >= 3
    ws = [torch.randn(r.shape, generator=g, dtype=torch.float64) for r in res_h]
    grads_h = torch.autograd.grad(sum((r * w).sum() for r, w in zip(res_h, ws)), leaves_h)
    grads_d = torch.autograd.grad(sum((r.double() * w.to(DEV)).sum() for r, w in zip(res_d, ws)), leaves_d)
    for k, (gd, gh) in enumerate(zip(grads_d, grads_h)):
        assert _rel(gd, gh) < 1e-5, (name, k, _rel(gd, gh))


def test_rk_tape_gradients_match_the_host_run(monkeypatch):
    "RKUltra with compute_scale=None takes the op tape (native.rk_step) under grad too; gradients match the float64 CPU run"
    monkeypatch.setattr(native, "mode", "always")
    make = lambda **kw: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=3, compute_scale=None, **kw)  # noqa: E731
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(SHAPE, generator=g, dtype=torch.float64)
    net_h, net_d = _net().double(), _net().to(DEV)
    xh, xd = x0.clone().requires_grad_(), x0.float().to(DEV).requires_grad_()
    before = native.launches
    out_d = _loop(make, xd, net_d)
    assert native.launches > before and out_d.grad_fn is not None
    out_h = _loop(make, xh, net_h)
    out_h.square().mean().backward()
    out_d.square().mean().backward()
    assert _rel(xd.grad, xh.grad) < 1e-5 and _rel(net_d.weight.grad, net_h.weight.grad) < 1e-5
