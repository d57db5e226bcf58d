"""Autograd through the device steps, host side (no GPU): the numbers the backward kernel is handed.

  * the fused step's transposition (a_k, b_k), with the rounded pair conversion folded in, equals torch autograd of the host executor
    (`lazy._host_evaluate`) on float64 CPU tensors;
  * the op tape's fold (native.fold) equals torch autograd of `native._run_host` for every sampler / order / model / dtype of the grammar
    the tape tests use, and no such tape holds an op without a linear gradient (tensor * tensor, tensor / tensor, number / tensor)."""

import zlib

import pytest
import torch
from cases import MODELS, SAMPLERS, SCHEDULES

from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.sampling import lazy, native
from skrample_amd.sampling import structured as PT


def _plan(c0, c1, chain, two: bool):
    plan = _hip.StepPlanC()
    plan.n_terms = len(c0)
    for k, (x, y) in enumerate(zip(c0, c1)):
        plan.coef0[k], plan.coef1[k] = x, y
    plan.chain = chain
    plan.out0_dtype = _hip.F64
    plan.out1_dtype = _hip.F64 if two else _hip.NONE
    return plan


def _leaves(n, shape=(2, 3, 4), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_() for _ in range(n)]


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_transposed_step_equals_autograd_of_the_host_executor(n, two):
    g = torch.Generator().manual_seed(10 * n + two)
    c0 = [float(v) for v in torch.randn(n, generator=g, dtype=torch.float64)]
    c1 = [float(v) for v in torch.randn(n, generator=g, dtype=torch.float64)]
    chain = 0.37 if two else 0.0
    xs = _leaves(n, seed=n)
    f0 = lazy.Lin({id(x): (x, c) for x, c in zip(xs, c0)}, xs[0].shape, xs[0].device)
    f1 = (f0.node() * chain + lazy.Lin({id(x): (x, c) for x, c in zip(xs, c1)}, xs[0].shape, xs[0].device)) if two else None
    outs = lazy._host_evaluate(None, f0, f1.expanded(keep=f0) if two else None, [torch.float64] * (2 if two else 1), True)
    gs = _leaves(len(outs), seed=99)
    grads = torch.autograd.grad(sum((o * w.detach()).sum() for o, w in zip(outs, gs)), xs)
    a, b = lazy.transposed(_plan(c0, c1, chain, two), None, n)
    for k in range(n):
        want = a[k] * gs[0].detach() + (b[k] * gs[1].detach() if two else 0)
        torch.testing.assert_close(grads[k], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("to_kind", [0, 1, 2, 3])
@pytest.mark.parametrize("from_kind", [0, 1, 2, 3])
def test_rounded_conversion_folds_into_the_transposition(to_kind, from_kind):
    "out0 = from_x(s, to_x(s, o)) (the Runge-Kutta wrapper's conversion) is affine: its derivative folds into a_0, a_1"
    k = [0.83, 1.7, 0.41, 2.3]
    s, o, extra = _leaves(3, seed=7)
    conv = lazy.RoundedConversion(s, o, to_kind, from_kind, k)
    f0 = lazy.Lin({id(s): (s, 0.0), id(o): (o, 0.0)}, s.shape, s.device)
    chain, cs, co, ce = -0.6, 0.25, 1.5, 0.75
    f1 = conv.node() * chain + lazy.Lin({id(s): (s, cs), id(o): (o, co), id(extra): (extra, ce)}, s.shape, s.device)
    outs = lazy._host_evaluate(conv, f0, f1, [torch.float64, torch.float64], True)
    g0, g1 = (t.detach() for t in _leaves(2, seed=11))
    grads = torch.autograd.grad((outs[0] * g0).sum() + (outs[1] * g1).sum(), [s, o, extra])
    a, b = lazy.transposed(_plan([0.0, 0.0, 0.0], [cs, co, ce], chain, True), lazy.conversion_gradient(to_kind, from_kind, k), 3)
    for k_, grad in enumerate(grads):
        torch.testing.assert_close(grad, a[k_] * g0 + b[k_] * g1, rtol=1e-12, atol=1e-12)


TAPE_SAMPLERS = [name for name in SAMPLERS if not name.startswith("spc")]  # (SPC is not recorded on a tape: test_native_tape.py refusals)
COMBOS = (("karras_scaled", "eps"), ("linear", "flow"), ("zsnr", "v"), ("scaled", "scalex"), ("scaled", "data"))


def _record(sampler, x, out, step, model, sched, noise, previous):
    packed = PT.SampleInput(x, out, step, noise)
    if type(sampler) is PT.UniPC:
        tape, res = native.record_unipc(sampler, packed, model, sched, previous, require_device=False)
    else:
        tape, res = native.record_stated(sampler, packed, model, sched, previous, require_device=False)
    return tape, res


def _walk(name, dtype, visit):
    "every step of short runs over the schedule / model combinations: visit(tape, results, sampler) -> the step's record"
    sampler_of = SAMPLERS[name][1]
    steps, shape = 6, (2, 3, 4, 4)
    for sname, mname in COMBOS:
        g = torch.Generator().manual_seed(zlib.crc32(f"grad/{name}/{sname}/{mname}".encode()))
        sampler, sched, model = sampler_of(), SCHEDULES[sname][1](), MODELS[mname][1]
        x = torch.randn(shape, generator=g).to(dtype)
        previous = []
        for i in range(steps - (1 if sname == "zsnr" else 0)):
            out = torch.randn(shape, generator=g).to(dtype)
            noise = torch.randn(shape, generator=g).to(dtype) if sampler.require_noise else None
            step = Step.from_int(i, steps)
            tape, res = _record(sampler, x, out, step, model, sched, noise, tuple(previous))
            vals = [t.detach() for t in native._run_host(tape, res)]
            visit(tape, res, (name, sname, mname, i))
            rec = PT.SKSamples(vals[0], vals[1], step, noise, vals[2]) if type(sampler) is PT.UniPC else PT.SKSamples(x, out, step, noise, vals[0])
            previous.append(rec)
            keep = sampler.require_previous
            previous = previous[max(len(previous) - keep, 0) :] if keep else []
            x = rec.final


@pytest.mark.parametrize("name", TAPE_SAMPLERS)
def test_tape_fold_equals_autograd_of_the_host_tape(name):
    def visit(tape, res, where):
        leaves = [t.detach().requires_grad_() for t in tape.leaves]
        tape.leaves = leaves
        outs = native._run_host(tape, res)
        g = torch.Generator().manual_seed(zlib.crc32(repr(where).encode()))
        ws = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
        grads = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, ws)), leaves, allow_unused=True)
        want = [torch.zeros_like(t) for t in leaves]
        for v, w in zip(res, ws):
            for leaf, c in native.fold(tape, v.n).items():
                want[leaf] = want[leaf] + c * w
        for k, grad in enumerate(grads):
            torch.testing.assert_close(grad if grad is not None else torch.zeros_like(leaves[k]), want[k], rtol=1e-9, atol=1e-12, msg=lambda m: f"{where} leaf {k}: {m}")

    _walk(name, torch.float64, visit)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize("name", TAPE_SAMPLERS)
def test_no_sampler_tape_holds_a_nonlinear_op(name, dtype):
    def visit(tape, res, where):
        held = [native._NONLINEAR[op[0]] for op in tape.ops if op[0] in native._NONLINEAR]
        assert not held, (where, held)

    _walk(name, dtype, visit)


def test_fold_refuses_a_nonlinear_op():
    x, y = torch.randn(2, 4, dtype=torch.float64), torch.randn(2, 4, dtype=torch.float64)
    tape = native.Tape(torch.float64, x.shape, x.device, require_device=False)
    prod = tape.leaf(x) * tape.leaf(y)
    with pytest.raises(_hip.SkrampleHipError, match="MUL"):
        native.fold(tape, prod.n)
    quot = 2.0 / tape.leaf(x)
    with pytest.raises(_hip.SkrampleHipError, match="RDIV_S"):
        native.fold(tape, quot.n)
    lin = tape.leaf(x) * 0.5 - tape.leaf(y) / 4.0 + 1.0
    assert native.fold(tape, lin.n) == {0: 0.5, 1: -0.25}


def test_grad_is_not_recorded_without_requires_grad():
    x = torch.randn(3)
    assert not lazy.grad_recorded(x, None, 1.0)
    w = x.clone().requires_grad_()
    assert lazy.grad_recorded(x, w)
    with torch.no_grad():
        assert not lazy.grad_recorded(w)


def _capture_host_tapes(monkeypatch):
    "every tape the host executor runs, with its results"
    seen = []
    run = native._run_host

    def spy(tape, results):
        seen.append((tape, list(results)))
        return run(tape, results)

    monkeypatch.setattr(native, "_run_host", spy)
    return seen, run


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
@pytest.mark.parametrize("order", [2, 3, 4])
def test_rk_wrapper_tapes_are_linear_and_fold_as_autograd(order, dtype, monkeypatch):
    """the Runge-Kutta wrapper with compute_scale=None records its stages on tapes (native.rk_step): none holds a nonlinear op, and on
    float64 leaves the fold equals torch autograd of the tape"""
    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS

    monkeypatch.setattr(native, "mode", "always")
    seen, run_host = _capture_host_tapes(monkeypatch)
    w = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=order, compute_scale=None)
    w.set_timesteps(4)
    g = torch.Generator().manual_seed(order)
    x = torch.randn(1, 2, 4, 4, generator=g).to(dtype)
    for t in w.timesteps:
        x = w.step(x * 0.5 + 0.1, t, x, return_dict=False)[0]
    assert seen
    for tape, res in list(seen):
        held = [native._NONLINEAR[op[0]] for op in tape.ops if op[0] in native._NONLINEAR]
        assert not held, held
        if dtype == torch.float64:
            leaves = [t.detach().requires_grad_() for t in tape.leaves]
            tape.leaves = leaves
            outs = run_host(tape, res)
            ws = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
            grads = torch.autograd.grad(sum((o * w_).sum() for o, w_ in zip(outs, ws)), leaves, allow_unused=True)
            for k, grad in enumerate(grads):
                want = sum((c * w_ for v, w_ in zip(res, ws) for leaf, c in native.fold(tape, v.n).items() if leaf == k), torch.zeros_like(leaves[k]))
                torch.testing.assert_close(grad if grad is not None else torch.zeros_like(leaves[k]), want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_functional_rk_tapes_are_linear(dtype, monkeypatch):
    "the functional Runge-Kutta samplers' tapes (native.step_tableau) hold no nonlinear op either"
    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from cases import fake_model

    seen, _run = _capture_host_tapes(monkeypatch)
    w = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=3, compute_scale=None)
    x = torch.randn(1, 2, 4, 4, generator=torch.Generator().manual_seed(4)).to(dtype)
    w.functional_sample_model(x, fake_model, 4)
    assert seen
    for tape, _res in seen:
        held = [native._NONLINEAR[op[0]] for op in tape.ops if op[0] in native._NONLINEAR]
        assert not held, held
