"""Autograd through masked (in-painting) steps on the device: skr_step_masked_backward_launch against skr_step_backward_launch (binary
masks), against float64 (soft masks), its two kernels against each other, its refusals; lazy._MaskedStepFunction under
torch.autograd.gradcheck; and SkrampleWrapperScheduler.set_inpaint loops differentiated on the device against the same loops on float64
CPU tensors with the blend written by hand.

The float64 bound of a gradient (per element; derived, not tuned):   2 (4 + 4) u_acc M  +  u_out |ref|  +  tiny_out
the form of test_masked_gpu.bound with n = 4: four rounded operations (1 - m, b * t, the fma, w * g) plus the fp32 rounding of the two
coefficients; M = (|c0 m| + |c1 (1 - m)|) |g|, u_acc = 2^-24 (fp32 arithmetic) or 2^-53, u_out / tiny_out by the gradient's dtype."""

import ctypes
import math

import numpy as np
import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U_OUT = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24, torch.float64: 2.0**-53}
TINY = {torch.bfloat16: 2.0**-133, torch.float16: 2.0**-24, torch.float32: 2.0**-149, torch.float64: 2.0**-1074}
OK, ERR_NULL, ERR_DTYPE, ERR_TERMS, ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5, 7
NAME = "skr_step_masked_backward_launch"

# (latents per sample, mask per sample, one mask for the whole batch): the table of tests/test_masked_gpu.py::SHAPES
SHAPES = {
    "wraps_twice_in_a_chunk": ((4, 32, 32), (1, 32, 32), False),
    "mask_spans_two_chunks": ((4, 64, 64), (1, 64, 64), False),
    "wraps_mid_chunk": ((4, 96, 96), (1, 96, 96), False),  # 18 chunks per sample: the bps_shift < 0 path
    "batch_stride_0": ((4, 64, 64), (1, 64, 64), True),
    "full_mask": ((4, 32, 32), (4, 32, 32), False),
    "sample_below_a_chunk": ((4, 16, 16), (1, 16, 16), False),  # general kernel
    "ragged": ((3, 24, 24), (1, 24, 24), False),  # general kernel
    "mask_numel_not_8": ((2, 5, 7), (1, 5, 7), False),  # general kernel
}
F64_SHAPES = ("wraps_twice_in_a_chunk", "ragged")
CASES = [(name, dt) for name in SHAPES for dt in (torch.bfloat16, torch.float16, torch.float32)] + [(name, torch.float64) for name in F64_SHAPES]
BATCH = {"wraps_mid_chunk": 1, "mask_spans_two_chunks": 2}  # (the others: 3)
COUNTS = (1, 4, 5, 8, 9, 16)  # every kernarg slot size (4 / 8 / 16) is filled and crossed


@pytest.fixture(scope="module", autouse=True)
def library():
    return _hip.load()


def bound(magnitude, ref, out_dtype, u_acc=2.0**-24):
    return 2 * (4 + 4) * u_acc * magnitude + U_OUT[out_dtype] * np.abs(ref) + TINY[out_dtype]


def f64(t):
    return t.detach().cpu().double().numpy()


class Problem:
    "an incoming gradient, a mask and the two coefficient lists of n gradients; with n >= 2 one operand has c1 == 0 and one c0 == 0"

    def __init__(self, name, dtype, n, soft, seed, grad_dtypes=None):
        unit, munit, whole = SHAPES[name]
        batch = BATCH.get(name, 3)
        self.shape, self.dtype, self.n = (batch, *unit), dtype, n
        gen = torch.Generator().manual_seed(seed)
        self.g = torch.randn(self.shape, generator=gen).to(dtype).to(DEV)
        pick = lambda: float((torch.rand((), generator=gen) * 1.9 + 0.1) * (1 if torch.rand((), generator=gen) < 0.5 else -1))  # noqa: E731  +-[0.1, 2]
        self.c0, self.c1 = [pick() for _ in range(n)], [pick() for _ in range(n)]
        if n >= 2:
            self.c1[0], self.c0[n - 1] = 0.0, 0.0  # absent from the known form / from the step form
        mshape = (1 if whole else batch, *munit)
        if soft:
            mask = torch.rand(mshape, generator=gen)
        else:
            mask = (torch.rand(mshape, generator=gen) < 0.5).float()
            mask[..., 0, :], mask[..., 1, :] = 1.0, 0.0  # a full row of each value
        self.mask = mask.to(dtype).to(DEV)
        self.mask_numel, self.batch_stride = lazy.mask_layout(mshape, self.shape)
        self.sample_numel = math.prod(unit)
        self.m_full = self.mask.expand(self.shape)  # (broadcast over the batch and the channels, as the kernel reads it)
        self.like = [lazy._Like(self.shape, d) for d in (grad_dtypes or [dtype] * n)]
        self.acc_f64 = dtype == torch.float64

    def masked(self):
        return lazy.launch_masked_backward(self.g, self.mask, self.mask_numel, self.batch_stride, self.c0, self.c1, self.like, self.sample_numel, self.acc_f64)

    def plain(self, coefs):
        "skr_step_backward_launch: coefs[k] * g"
        return lazy.launch_backward(self.g, None, coefs, [0.0] * self.n, self.like, self.acc_f64)

    def check_against_float64(self, grads, what):
        m, g = f64(self.m_full), f64(self.g)
        u_acc = 2.0**-53 if self.acc_f64 else 2.0**-24
        worst = 0.0
        for k, got in enumerate(grads):
            ref = (self.c0[k] * m + self.c1[k] * (1 - m)) * g
            mag = (np.abs(self.c0[k] * m) + np.abs(self.c1[k] * (1 - m))) * np.abs(g)
            tol = bound(mag, ref, got.dtype, u_acc)
            err = np.abs(f64(got) - ref)
            worst = max(worst, float((err / tol).max()))
            assert got.dtype == self.like[k].dtype and tuple(got.shape) == self.shape
            assert (err <= tol).all(), (what, k, float((err / tol).max()))
        return worst


@pytest.mark.parametrize("name,dtype", CASES)
def test_binary_masks_give_the_plain_backward(name, dtype):
    "where m == 1: skr_step_backward_launch with a = c0; where m == 0: with a = c1 (the yardstick is the existing kernel)"
    for n in COUNTS:
        p = Problem(name, dtype, n, soft=False, seed=100 + n)
        got, step, known = p.masked(), p.plain(p.c0), p.plain(p.c1)
        keep = p.m_full == 1
        assert keep.any() and (~keep).any() and ((p.m_full == 0) | keep).all()
        for k in range(n):
            want = torch.where(keep, step[k], known[k])
            assert torch.equal(got[k], want), (name, dtype, n, k, int((got[k] != want).sum()))  # (values: signed zeros compare equal)


@pytest.mark.parametrize("name,dtype", CASES)
def test_soft_masks_against_float64(name, dtype):
    for n in COUNTS:
        p = Problem(name, dtype, n, soft=True, seed=200 + n)
        worst = p.check_against_float64(p.masked(), (name, dtype, n))
        print(f"{name} {dtype} n={n}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_vector_kernel_equals_general_kernel(dtype, library):
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    for n in COUNTS:
        p = Problem("wraps_twice_in_a_chunk", dtype, n, soft=True, seed=300 + n)
        fast = p.masked()
        try:
            assert library.skr_set_tuning(b"one_trip", 0) == 0
            general = p.masked()
        finally:
            library.skr_set_tuning(b"one_trip", 1)
        for k in range(n):
            assert torch.equal(fast[k].view(bits), general[k].view(bits)), (dtype, n, k)


@pytest.mark.parametrize("name", ["wraps_twice_in_a_chunk", "ragged"])
def test_two_dtype_groups_through_the_general_kernel(name):
    "two fp32 and two bf16 gradients of an fp32 incoming gradient"
    p = Problem(name, torch.float32, 4, soft=True, seed=400, grad_dtypes=[torch.float32, torch.float32, torch.bfloat16, torch.bfloat16])
    worst = p.check_against_float64(p.masked(), name)
    print(f"{name} fp32 + bf16 gradients: worst error / bound {worst:.3f}")


def test_error_codes(library):
    "argument checks only: every call but the control is refused before anything is launched"
    p = Problem("wraps_twice_in_a_chunk", torch.bfloat16, 3, soft=False, seed=1)
    grads = [torch.zeros(p.shape, dtype=p.dtype, device=DEV) for _ in range(3)]
    numel, sn, mn = p.g.numel(), p.sample_numel, p.mask_numel
    stream = _hip.current_stream_ptr(DEV)
    arr = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in grads])
    entry = getattr(library, NAME)

    def call(plan=True, g=p.g.data_ptr(), mask_ptr=p.mask.data_ptr(), mask_dtype=_hip.BF16, mask_numel=mn, batch_stride=mn, out=arr, n=numel, sample_numel=sn, desc=True, **fields):
        pl = _hip.StepGradPlanC()
        pl.n_grads = pl.n_group_a = 3
        pl.dtype_a = pl.dtype_b = pl.g0_dtype = _hip.BF16
        pl.g1_dtype = _hip.NONE
        for k in range(3):
            pl.a[k], pl.b[k] = p.c0[k], p.c1[k]
        for key, value in fields.items():
            setattr(pl, key, value)
        d = _hip.StepMaskC(mask_ptr, mask_dtype, 0, mask_numel, batch_stride)
        return entry(ctypes.byref(pl) if plan else None, g, ctypes.byref(d) if desc else None, out, n, sample_numel, stream)

    assert call(plan=False) == ERR_NULL
    assert call(desc=False) == ERR_NULL
    assert call(g=None) == ERR_NULL
    assert call(out=None) == ERR_NULL
    assert call(mask_ptr=None) == ERR_NULL
    assert call(out=(ctypes.c_void_p * 3)(grads[0].data_ptr(), None, grads[2].data_ptr())) == ERR_NULL
    assert call(g0_dtype=9) == ERR_DTYPE
    assert call(dtype_a=_hip.NONE) == ERR_DTYPE
    assert call(n_group_a=2, dtype_b=17) == ERR_DTYPE
    assert call(mask_dtype=5) == ERR_DTYPE
    assert call(n_grads=0, n_group_a=0) == ERR_TERMS
    assert call(n_grads=_hip.ROW_TERMS + 1, n_group_a=_hip.ROW_TERMS + 1) == ERR_TERMS
    assert call(n_group_a=4) == ERR_TERMS
    assert call(g=p.g.data_ptr() + 2) == ERR_ALIGN
    assert call(mask_ptr=p.mask.data_ptr() + 8) == ERR_ALIGN
    assert call(out=(ctypes.c_void_p * 3)(grads[0].data_ptr(), grads[1].data_ptr() + 2, grads[2].data_ptr())) == ERR_ALIGN
    assert call(mask_numel=0) == ERR_SHAPE
    assert call(mask_numel=-8) == ERR_SHAPE
    assert call(mask_numel=mn - 8, batch_stride=mn - 8) == ERR_SHAPE  # does not divide sample_numel
    assert call(sample_numel=sn - 8) == ERR_SHAPE  # does not divide numel
    assert call(sample_numel=0) == ERR_SHAPE
    assert call(batch_stride=8) == ERR_SHAPE
    assert call(batch_stride=-mn) == ERR_SHAPE
    assert call(n=-1) == ERR_SHAPE
    assert call(g1_dtype=_hip.BF16) == ERR_UNSUPPORTED
    assert call(mask_dtype=_hip.F64) == ERR_UNSUPPORTED  # an fp64 mask without acc_f64
    assert call(n=0) == OK  # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert not any(t.any() for t in grads)  # nothing was written by any of them
    assert call() == OK  # the control
    torch.cuda.synchronize()
    assert all(t.any() for t in grads)


# ---- lazy.evaluate_masked and the scheduler wrapper under autograd -------------------------------------------------------------------
def _dev64(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).to(DEV).requires_grad_()


def test_gradcheck_evaluate_masked():
    "a soft (2,1,8,8) mask over (2,2,8,8); `orig` is shared between the two forms, `nz` is in the known form only"
    x, o, orig, nz = (_dev64(2, 2, 8, 8, seed=s) for s in (1, 2, 3, 4))
    mask = torch.rand(2, 1, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(DEV)

    def f(x, o, orig, nz):
        form = lazy.lift(x) * 1.25 + lazy.lift(o) * -0.75 + lazy.lift(orig) * 0.3
        known = lazy.lift(orig) * 0.9 + lazy.lift(nz) * 0.45
        return lazy.evaluate_masked(form, known, mask, dtype=torch.float64)

    assert f(x, o, orig, nz).grad_fn is not None
    assert torch.autograd.gradcheck(f, (x, o, orig, nz), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_gradcheck_wrapper_inpaint_sde_steps():
    "three DPM-2 SDE steps under set_inpaint, noise drawn in the kernel from seeded generators, compute_scale=float64"
    shape = (2, 1, 4, 8)
    x, o0, o1, o2, orig, nz = (_dev64(*shape, seed=10 + s) for s in range(6))
    mask = torch.rand(2, 1, 4, 8, generator=torch.Generator().manual_seed(7), dtype=torch.float64).to(DEV)

    def f(x, o0, o1, o2, orig, nz):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), compute_scale=torch.float64)
        w.set_timesteps(3)
        w.set_inpaint(mask, orig, nz)
        gens = [torch.Generator().manual_seed(s) for s in (11, 12)]
        for t, o in zip(w.timesteps, (o0, o1, o2)):
            x = w.step(o, t, x, generator=gens, return_dict=False)[0]
        return x

    assert f(x, o0, o1, o2, orig, nz).grad_fn is not None
    assert torch.autograd.gradcheck(f, (x, o0, o1, o2, orig, nz), eps=1e-6, atol=1e-6, rtol=1e-5)


SAMPLERS = {
    "euler": lambda: PT.Euler(),
    "dpm2": lambda: PT.DPM(order=2),
    "adams4": lambda: PT.Adams(order=4),
    "unip3": lambda: PT.UniP(order=3),
    "unipc3": lambda: PT.UniPC(order=3),  # two launches: its own step, then the blend
    "spc": lambda: PT.SPC(),
}
STEPS = 5


def _wrapper(name):
    return PD.SkrampleWrapperScheduler(SAMPLERS[name](), PS.Karras(PS.Scaled()))


def _net(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Conv2d(4, 4, 3, padding=1)
    with torch.no_grad():
        net.weight.mul_(0.3)
    return net


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def _binary_mask(shape, gen):
    mask = (torch.rand((shape[0], 1, *shape[2:]), generator=gen) < 0.5).double()
    mask[:, :, 0, :], mask[:, :, 1, :] = 1.0, 0.0
    return mask


def _host_loop(name, x, net, mask, original, noise):
    "the same wrapper class without set_inpaint, the blend written by hand after every step"
    w = _wrapper(name)
    w.set_timesteps(STEPS)
    for i, t in enumerate(w.timesteps):
        x = w.step(net(x), t, x, return_dict=False)[0]
        known = w.add_noise(original, noise, w.timesteps[i + 1 : i + 2]) if i + 1 < STEPS else original
        x = mask * x + (1 - mask) * known
    return x


def _device_loop(name, x, net, mask, original, noise):
    w = _wrapper(name)
    w.set_timesteps(STEPS)
    w.set_inpaint(mask, original, noise)
    for t in w.timesteps:
        x = w.step(net(x), t, x, return_dict=False)[0]
    return x


@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (2, 4, 32, 32)], ids=["general", "one_trip"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_wrapper_inpaint_loop_gradients_match_the_host_run(name, shape):
    """fp32 on the device against float64 on the host: gradients of the initial latents, the network's weight and bias, original_samples
    and noise, by the relative-norm measure and the 1e-5 limit of test_autograd_gpu.test_wrapper_loop_gradients_match_the_host_run"""
    gen = torch.Generator().manual_seed(1)
    x0, target, original, noise = (torch.randn(shape, generator=gen, dtype=torch.float64) for _ in range(4))
    mask = _binary_mask(shape, gen)
    net_h, net_d = _net().double(), _net().to(DEV)
    host = [t.clone().requires_grad_() for t in (x0, original, noise)]
    device = [t.float().to(DEV).requires_grad_() for t in (x0, original, noise)]
    out_h = _host_loop(name, host[0], net_h, mask, host[1], host[2])
    out_d = _device_loop(name, device[0], net_d, mask.float().to(DEV), device[1], device[2])
    assert out_d.grad_fn is not None and out_d.is_cuda and out_d.dtype == torch.float32
    ((out_h - target) ** 2).mean().backward()
    ((out_d - target.float().to(DEV)) ** 2).mean().backward()
    pairs = {"latents": (device[0].grad, host[0].grad), "original_samples": (device[1].grad, host[1].grad), "noise": (device[2].grad, host[2].grad),
             "weight": (net_d.weight.grad, net_h.weight.grad), "bias": (net_d.bias.grad, net_h.bias.grad)}  # fmt: skip
    for what, (got, want) in pairs.items():
        assert got is not None and want is not None, (name, what)
        print(f"{name} {shape} {what}: relative error {_rel(got, want):.3e}")
    for what, (got, want) in pairs.items():
        assert _rel(got, want) < 1e-5, (name, what, _rel(got, want))


@pytest.mark.parametrize("name", ["dpm2", "unipc3"])
def test_forward_bits_under_autograd_are_those_without(name):
    shape = (2, 4, 32, 32)
    gen = torch.Generator().manual_seed(2)
    x, out, original, noise = (torch.randn(shape, generator=gen).bfloat16().to(DEV) for _ in range(4))
    mask = _binary_mask(shape, gen).to(DEV)

    def two_steps(record):
        w = _wrapper(name)
        w.set_timesteps(STEPS)
        w.set_inpaint(mask, original, noise)
        y = x.clone().requires_grad_(record)
        results = []
        for t in w.timesteps[:2]:
            y = w.step(out, t, y, return_dict=False)[0]
            results.append(y)
        return results

    recorded = two_steps(True)
    with torch.no_grad():
        plain = two_steps(True)
    for a, b in zip(recorded, plain):
        assert a.grad_fn is not None and b.grad_fn is None and not b.requires_grad
        assert a.dtype == torch.bfloat16 and torch.equal(a.detach().view(torch.int16), b.view(torch.int16)), name


def test_one_masked_backward_launch_per_step_and_no_buffer_for_operands_without_grad(monkeypatch):
    shape = (2, 4, 32, 32)
    gen = torch.Generator().manual_seed(3)
    x, out, out_before, original, noise = (torch.randn(shape, generator=gen).to(DEV) for _ in range(5))
    mask = _binary_mask(shape, gen).float().to(DEV)
    calls = []
    launcher = lazy.launch_masked_backward

    def counted(g, mask, mask_numel, batch_stride, a, b, like, sample_numel, acc_f64):
        grads = launcher(g, mask, mask_numel, batch_stride, a, b, like, sample_numel, acc_f64)
        calls.append(len(grads))
        return grads

    monkeypatch.setattr(lazy, "launch_masked_backward", counted)
    w = _wrapper("dpm2")
    w.set_timesteps(STEPS)
    w.set_inpaint(mask, original, noise)
    with torch.no_grad():
        y = w.step(out_before, w.timesteps[0], x, return_dict=False)[0]
    # the second step reads five operands (sample, model output, the first step's output, original, noise); three require grad
    y.requires_grad_(), out.requires_grad_(), original.requires_grad_()
    z = w.step(out, w.timesteps[1], y, return_dict=False)[0]
    assert z.grad_fn is not None and not calls
    z.sum().backward()
    assert calls == [3], calls
    assert y.grad is not None and out.grad is not None and original.grad is not None and noise.grad is None and out_before.grad is None


def test_refusals_and_no_grad_on_the_device():
    shape = (2, 4, 16, 16)
    gen = torch.Generator().manual_seed(4)
    x, original = (torch.randn(shape, generator=gen).to(DEV).requires_grad_() for _ in range(2))
    mask = torch.rand((2, 1, 16, 16), generator=gen).to(DEV)
    form, known = lazy.lift(x) * 0.5, lazy.lift(original) * 0.25
    with pytest.raises(lazy.SkrampleHipError, match="mask of a masked step has no gradient"):
        lazy.evaluate_masked(form, known, mask.clone().requires_grad_())
    with torch.no_grad():  # runs as before: the plain launch, a detached result
        detached = lazy.evaluate_masked(form, known, mask)
    assert detached.grad_fn is None and not detached.requires_grad
    recorded = lazy.evaluate_masked(form, known, mask)
    assert recorded.grad_fn is not None and torch.equal(recorded.detach(), detached)


def test_history_alias_guards_deepcopy_and_prediction_behave_as_without_autograd():
    """masked Adams-4 steps (three history records) through a Conv2d, every alias_history setting, on a deepcopy of a scheduler that has
    in-painting set: prev_sample and pred_original_sample have the bits of the run under torch.no_grad(), and the latents' gradient does
    not depend on the setting"""
    import copy

    shape = (2, 4, 32, 32)
    gen = torch.Generator().manual_seed(6)
    x0, original, noise = (torch.randn(shape, generator=gen).to(DEV) for _ in range(3))
    mask = _binary_mask(shape, gen).float().to(DEV)
    grads = []
    for alias in (True, False, "auto"):
        net = _net().to(DEV)
        template = PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.Karras(PS.Scaled()), alias_history=alias)
        template.set_inpaint(mask, original, noise)

        def loop(x):
            w = copy.deepcopy(template)  # (carries the three in-painting tensors along)
            w.set_timesteps(STEPS)
            predictions = []
            for t in w.timesteps:
                x, pred = w.step(net(x), t, x, return_dict=False)
                predictions.append(pred.materialize() if isinstance(pred, lazy.LazyTensor) else pred)
            return x, predictions

        with torch.no_grad():
            plain, plain_predictions = loop(x0)
        x = x0.clone().requires_grad_()
        got, predictions = loop(x)
        assert got.grad_fn is not None and torch.equal(got.detach(), plain), alias
        for a, b in zip(predictions, plain_predictions):
            assert torch.equal(a.detach(), b), alias
        got.square().mean().backward()
        grads.append((x.grad.clone(), net.weight.grad.clone()))
    # the latents' gradient is the end of the chain through every step: its bits pin every gradient the steps hand back.  The weight
    # gradient is a reduction made by the convolution library, whose summation order is not fixed at this size: the 1e-5 of the loops above
    for gx, gw in grads[1:]:
        assert torch.equal(gx, grads[0][0]) and _rel(gw, grads[0][1]) < 1e-5
