"""Masked steps (in-painting) on the device: skr_step_launch_masked against skr_step_launch (bit properties with binary masks), against
float64 (soft masks), its two kernels against each other, its refusals, and SkrampleWrapperScheduler.set_inpaint / clear_inpaint.

The float64 bound (per element; derived, not tuned):   2 (n + 4) u_acc M  +  u_out |ref|  +  tiny_out
n operands (+1 with noise), u_acc = 2^-24 (fp32 accumulation) or 2^-53, M = |m| (sum |coef0_k x_k| + |zeta0 N|) + |1 - m| sum |coef1_k x_k|,
u_out = 2^-8 / 2^-11 / 2^-24 / 2^-53 by output dtype, tiny_out its smallest subnormal: one rounding for every coefficient's conversion, one
for every fma, three for the blend; the factor 2 covers the second-order terms."""

import ctypes
import math

import numpy as np
import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.common import Point
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
U_OUT = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24, torch.float64: 2.0**-53}
TINY = {torch.bfloat16: 2.0**-133, torch.float16: 2.0**-24, torch.float32: 2.0**-149, torch.float64: 2.0**-1074}
OK, ERR_NULL, ERR_DTYPE, ERR_TERMS, ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5, 7


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def bound(n, magnitude, ref, out_dtype, u_acc=2.0**-24):
    return 2 * (n + 4) * u_acc * magnitude + U_OUT[out_dtype] * np.abs(ref) + TINY[out_dtype]


def f64(t):
    return t.detach().cpu().double().numpy()


# (latents per sample, mask per sample or None for a full mask, one mask for the whole batch, what it exercises)
SHAPES = {
    "wraps_twice_in_a_chunk": ((4, 32, 32), (1, 32, 32), False),
    "mask_spans_two_chunks": ((4, 64, 64), (1, 64, 64), False),
    "wraps_mid_chunk": ((4, 96, 96), (1, 96, 96), False),  # 18 chunks per sample, the mask wraps every 4.5
    "batch_stride_0": ((4, 64, 64), (1, 64, 64), True),
    "full_mask": ((4, 32, 32), (4, 32, 32), False),
    "sample_below_a_chunk": ((4, 16, 16), (1, 16, 16), False),  # general kernel
    "ragged": ((3, 24, 24), (1, 24, 24), False),  # general kernel
    "mask_numel_not_8": ((2, 5, 7), (1, 5, 7), False),  # general kernel; 70 elements per sample: no in-kernel noise either
}
F64_SHAPES = ("wraps_twice_in_a_chunk", "ragged")
CASES = [(name, dt) for name in SHAPES for dt in (torch.bfloat16, torch.float16, torch.float32)] + [(name, torch.float64) for name in F64_SHAPES]
BATCH = {"wraps_mid_chunk": 1, "mask_spans_two_chunks": 2}  # (the others: 3)


def make_plan(n, dtype, coef0, coef1, sample_numel, noise=None):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = _hip.DTYPE_CODE[dtype]
    plan.dtype_b = _hip.F64 if dtype == torch.float64 else _hip.F32
    plan.out1_dtype = _hip.NONE
    plan.acc_f64 = 1 if dtype == torch.float64 else 0
    for k in range(n):
        plan.coef0[k], plan.coef1[k] = coef0[k], coef1[k]
    plan.sample_numel = sample_numel
    if noise is not None:
        plan.noise_mode, plan.zeta0, plan.stream0 = 1, noise[1], noise[2]
    return plan


def raw_masked(plan, ops, out, mask, mask_numel, batch_stride, seeds, numel):
    arr = (ctypes.c_void_p * max(len(ops), 1))(*[t.data_ptr() for t in ops])
    desc = _hip.StepMaskC(mask.data_ptr(), _hip.DTYPE_CODE[mask.dtype], 0, mask_numel, batch_stride)
    return _hip.load().skr_step_launch_masked(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), seeds.data_ptr() if seeds is not None else None, numel, _hip.current_stream_ptr(out.device))


def plain_step(ops, coefs, dtype, shape, noise, dev):
    "skr_step_launch of one form over exactly `ops`"
    plan = make_plan(len(ops), dtype, coefs, [0.0] * len(ops), math.prod(shape[1:]), noise)
    out = torch.empty(shape, dtype=dtype, device=dev)
    _hip.launch_step(plan, ops, out, None, noise[0] if noise is not None else None, out.numel(), dev)
    return out


class Problem:
    "operands, coefficients and a mask for one (shape, dtype, operand count): the known form shares operand n-2 with the step form"

    def __init__(self, name, dtype, n, dev, soft, seed):
        unit, munit, whole = SHAPES[name]
        batch = BATCH.get(name, 3)
        self.shape, self.dtype, self.n, self.dev = (batch, *unit), dtype, n, dev
        g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(self.shape, generator=g).to(dtype).to(dev) for _ in range(n)]
        pick = lambda: float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # noqa: E731  +-[0.1, 2]
        self.coef0 = [pick() for _ in range(n - 1)] + [0.0]
        self.coef1 = [0.0] * (n - 2) + [pick(), pick()]
        mshape = (1 if whole else batch, *munit)
        if soft:
            mask = torch.rand(mshape, generator=g)
        else:
            mask = (torch.rand(mshape, generator=g) < 0.5).float()
            mask[..., 0, :], mask[..., 1, :] = 1.0, 0.0  # a full row of each value
        self.mask = mask.to(dtype).to(dev)
        self.mask_numel, self.batch_stride = lazy.mask_layout(mshape, self.shape)
        assert self.mask_numel == math.prod(munit) and self.batch_stride == (0 if whole or batch == 1 else self.mask_numel)
        self.sample_numel = math.prod(unit)
        self.seeds = torch.tensor([11, 22, 33][:batch], dtype=torch.int64, device=dev)
        self.m_full = self.mask.expand(self.shape)  # (broadcast over the batch and the channels, as the kernel reads it)

    def noise(self, on):
        return (self.seeds, 0.7, 3 * 256 + 1) if on and self.sample_numel % 8 == 0 else None

    def masked(self, noise):
        plan = make_plan(self.n, self.dtype, self.coef0, self.coef1, self.sample_numel, noise)
        out = torch.empty(self.shape, dtype=self.dtype, device=self.dev)
        _hip.launch_step_masked(plan, self.ops, out, self.mask, self.mask_numel, self.batch_stride, noise[0] if noise is not None else None, out.numel(), self.dev)
        return out


@pytest.mark.parametrize("name,dtype", CASES)
def test_binary_masks_give_the_bits_of_the_plain_step_launches(name, dtype, dev):
    "where m == 1: skr_step_launch of the step form (with its noise); where m == 0: skr_step_launch of the known form over exactly its operands"
    for n in (2, 5, 12):
        for noisy in (False, True):
            p = Problem(name, dtype, n, dev, soft=False, seed=100 + n)
            noise = p.noise(noisy)
            if noisy and noise is None:
                continue
            got = p.masked(noise)
            step = plain_step(p.ops, p.coef0, dtype, p.shape, noise, dev)
            known = plain_step(p.ops[n - 2 :], p.coef1[n - 2 :], dtype, p.shape, None, dev)
            keep = p.m_full == 1
            assert keep.any() and (~keep).any() and ((p.m_full == 0) | keep).all()
            want = torch.where(keep, step, known)
            bits = torch.int16 if dtype in (torch.bfloat16, torch.float16) else (torch.int32 if dtype == torch.float32 else torch.int64)
            assert torch.equal(got.view(bits), want.view(bits)), (name, dtype, n, noisy, int((got.view(bits) != want.view(bits)).sum()))


def test_a_noisy_launch_over_samples_that_are_no_multiple_of_8_is_refused_as_skr_step_launch_refuses_it(dev):
    p = Problem("mask_numel_not_8", torch.float32, 2, dev, soft=False, seed=5)
    noise = (p.seeds, 0.7, 9)
    plan = make_plan(2, torch.float32, p.coef0, p.coef1, p.sample_numel, noise)
    out = torch.zeros(p.shape, device=dev)
    assert raw_masked(plan, p.ops, out, p.mask, p.mask_numel, p.batch_stride, p.seeds, out.numel()) == ERR_UNSUPPORTED
    arr = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in p.ops])
    assert _hip.load().skr_step_launch(ctypes.byref(plan), arr, out.data_ptr(), None, p.seeds.data_ptr(), out.numel(), _hip.current_stream_ptr(dev)) == ERR_UNSUPPORTED


@pytest.mark.parametrize("name,dtype", CASES)
def test_soft_masks_against_float64(name, dtype, dev):
    u_acc = 2.0**-53 if dtype == torch.float64 else 2.0**-24
    for n in (2, 5, 12):
        for noisy in (False, True):
            p = Problem(name, dtype, n, dev, soft=True, seed=200 + n)
            noise = p.noise(noisy)
            if noisy and noise is None:
                continue
            got = f64(p.masked(noise))
            m = f64(p.m_full)
            xs = [f64(t) for t in p.ops]
            s_terms = [c * x for c, x in zip(p.coef0, xs)]
            if noise is not None:
                z = lazy.PhiloxNoise(noise[0], noise[2], p.shape, dev).realize(torch.float32)
                s_terms.append(noise[1] * f64(z))
            k_terms = [c * x for c, x in zip(p.coef1, xs)]
            ref = m * sum(s_terms) + (1 - m) * sum(k_terms)
            mag = np.abs(m) * sum(np.abs(t) for t in s_terms) + np.abs(1 - m) * sum(np.abs(t) for t in k_terms)
            tol = bound(n + (1 if noise is not None else 0), mag, ref, dtype, u_acc)
            err = np.abs(got - ref)
            print(f"{name} {dtype} n={n} noise={noise is not None}: worst error / bound {float((err / tol).max()):.3f}")
            assert got.shape == ref.shape and (err <= tol).all(), (name, dtype, n, noisy, float((err / tol).max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_vector_kernel_equals_general_kernel(dtype, dev):
    lib = _hip.load()
    for n in (2, 5, 12):
        for noisy in (False, True):
            p = Problem("wraps_twice_in_a_chunk", dtype, n, dev, soft=True, seed=300 + n)
            fast = p.masked(p.noise(noisy))
            try:
                assert lib.skr_set_tuning(b"one_trip", 0) == 0
                general = p.masked(p.noise(noisy))
            finally:
                lib.skr_set_tuning(b"one_trip", 1)
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            assert torch.equal(fast.view(bits), general.view(bits)), (dtype, n, noisy)


def test_error_codes(dev):
    "argument checks only: every call below is refused before anything is launched"
    p = Problem("wraps_twice_in_a_chunk", torch.bfloat16, 3, dev, soft=False, seed=1)
    out = torch.zeros(p.shape, dtype=p.dtype, device=dev)
    numel, sn, mn = out.numel(), p.sample_numel, p.mask_numel
    lib = _hip.load()
    stream = _hip.current_stream_ptr(dev)
    arr = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in p.ops])

    def call(plan=None, inputs=arr, out_ptr=out.data_ptr(), mask_ptr=p.mask.data_ptr(), mask_dtype=_hip.BF16, mask_numel=mn, batch_stride=mn, seeds=None, n=numel, desc=True, **fields):
        if plan is None:
            plan = make_plan(3, p.dtype, p.coef0, p.coef1, sn)
        for key, value in fields.items():
            setattr(plan, key, value)
        d = _hip.StepMaskC(mask_ptr, mask_dtype, 0, mask_numel, batch_stride)
        return lib.skr_step_launch_masked(ctypes.byref(plan) if plan is not False else None, inputs, out_ptr, ctypes.byref(d) if desc else None, seeds, n, stream)

    assert call(plan=False) == ERR_NULL and call(desc=False) == ERR_NULL
    assert call(inputs=None) == ERR_NULL and call(out_ptr=None) == ERR_NULL and call(mask_ptr=None) == ERR_NULL
    assert call(inputs=(ctypes.c_void_p * 3)(p.ops[0].data_ptr(), None, p.ops[2].data_ptr())) == ERR_NULL
    assert call(noise_mode=1, zeta0=0.5, seeds=None) == ERR_NULL  # a draw without seeds
    assert call(mask_numel=0) == ERR_SHAPE and call(mask_numel=-8) == ERR_SHAPE
    assert call(mask_numel=mn - 8, batch_stride=mn - 8) == ERR_SHAPE  # does not divide sample_numel
    assert call(sample_numel=sn - 8) == ERR_SHAPE and call(sample_numel=0) == ERR_SHAPE  # does not divide numel / missing
    assert call(batch_stride=8) == ERR_SHAPE and call(batch_stride=-mn) == ERR_SHAPE
    assert call(n=-1) == ERR_SHAPE
    assert call(inputs=(ctypes.c_void_p * 3)(p.ops[0].data_ptr(), p.ops[1].data_ptr() + 2, p.ops[2].data_ptr())) == ERR_ALIGN
    assert call(out_ptr=out.data_ptr() + 2) == ERR_ALIGN and call(mask_ptr=p.mask.data_ptr() + 8) == ERR_ALIGN
    assert call(out1_dtype=_hip.BF16) == ERR_UNSUPPORTED and call(chain=0.5) == ERR_UNSUPPORTED and call(zeta1=0.5) == ERR_UNSUPPORTED
    assert call(convert_to=1) == ERR_UNSUPPORTED and call(convert_from=2) == ERR_UNSUPPORTED
    assert call(n_terms=17, n_group_a=17) == ERR_TERMS and call(n_group_a=4) == ERR_TERMS
    assert call(mask_dtype=_hip.F64) == ERR_DTYPE and call(out0_dtype=_hip.F16) == ERR_DTYPE and call(dtype_a=_hip.F64) == ERR_DTYPE
    assert call(n=0) == OK  # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert not out.any()  # nothing was written by any of them


# ---- the scheduler wrapper -----------------------------------------------------------------------------------------------------------
ONE_LAUNCH = {
    "euler": lambda: PT.Euler(),
    "dpm2": lambda: PT.DPM(order=2),
    "adams3": lambda: PT.Adams(order=3),
    "unip2": lambda: PT.UniP(order=2),
}
TWO_LAUNCH = {"unipc2": lambda: PT.UniPC(order=2), "spc": lambda: PT.SPC()}
SHAPE, STEPS = (2, 4, 32, 32), 6


def inpaint_inputs(dev, seed):
    g = torch.Generator().manual_seed(seed)
    x, orig, nz = (torch.randn(SHAPE, generator=g).bfloat16().to(dev) for _ in range(3))
    outs = [torch.randn(SHAPE, generator=g).bfloat16().to(dev) for _ in range(STEPS)]
    mask = torch.rand((2, 1, 32, 32), generator=g) < 0.5
    mask[:, :, 0, :], mask[:, :, 1, :] = True, False
    return x, orig, nz, outs, mask.to(dev)


def compare_with_the_unfused_lines(sampler, launches_per_step, dev):
    """step() under set_inpaint against step() + add_noise() + the blend lines on a second wrapper of the same configuration.  Where the
    step's result is kept (m == 1) the two agree bit for bit; elsewhere the blend lines are evaluated in float64 on the stored values and
    the bound applies with the known form's own n = 2 and M = |a orig| + |b noise| (a, b: Point.add_noise's alpha and sigma of the next step)."""
    make = lambda: PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled()))  # noqa: E731
    masked, plain = make(), make()
    masked.set_timesteps(STEPS), plain.set_timesteps(STEPS)
    x, orig, nz, outs, mask = inpaint_inputs(dev, 21)
    masked.set_inpaint(mask, orig, nz)
    assert masked._inpaint[0].dtype == torch.bfloat16
    keep = mask.expand(SHAPE)
    ts = plain.timesteps.tolist()
    xa = x
    for i, t in enumerate(ts):
        _hip.trace = []
        try:
            got, pred_a = masked.step(outs[i], t, xa, return_dict=False)
            launches = len(_hip.trace)
        finally:
            _hip.trace = None
        assert launches == launches_per_step, (i, launches)
        prev, pred_b = plain.step(outs[i], t, xa, return_dict=False)
        assert got.dtype == torch.bfloat16 and torch.equal(got[keep].view(torch.int16), prev[keep].view(torch.int16)), i
        if i + 1 < STEPS:
            point = Point(*plain.schedule_np[i + 1])
            a, b = float(point.alpha), float(point.sigma)
            known = f64(plain.add_noise(orig.double(), nz.double(), plain.timesteps[i + 1 : i + 2]))
            assert np.allclose(known, a * f64(orig) + b * f64(nz), rtol=1e-12, atol=0)  # (the same algebra, in float64)
            mag = abs(a) * np.abs(f64(orig)) + abs(b) * np.abs(f64(nz))
        else:
            known, mag = f64(orig), np.abs(f64(orig))
            assert torch.equal(got[~keep].view(torch.int16), orig[~keep].view(torch.int16))  # after the last step: the original itself
        away = ~keep.cpu().numpy()
        err = np.abs(f64(got) - known)[away]
        assert (err <= bound(2, mag, known, torch.bfloat16)[away]).all(), (i, float(err.max()))
        pred_a, pred_b = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (pred_a, pred_b))
        assert torch.equal(pred_a, pred_b)  # pred_original_sample is unchanged
        xa = got
    assert masked._fast_hits == 0


@pytest.mark.parametrize("name", sorted(ONE_LAUNCH))
def test_wrapper_masked_step_is_one_launch(name, dev):
    compare_with_the_unfused_lines(ONE_LAUNCH[name], 1, dev)


@pytest.mark.parametrize("name", sorted(TWO_LAUNCH))
def test_wrapper_two_output_samplers_blend_in_a_second_launch(name, dev):
    compare_with_the_unfused_lines(TWO_LAUNCH[name], 2, dev)


def run(w, x, outs):
    w.set_timesteps(len(outs))
    traj = []
    for i, t in enumerate(w.timesteps.tolist()):
        x = w.step(outs[i], t, x, return_dict=False)[0]
        traj.append(x)
    return traj


def test_clear_inpaint_restores_the_replayed_fast_path(dev):
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))  # noqa: E731
    cleared, never = make(), make()
    never.fast_steps = False
    x, orig, nz, outs, mask = inpaint_inputs(dev, 23)
    want = run(never, x, outs)
    cleared.set_inpaint(mask, orig, nz)
    masked = run(cleared, x, outs)
    assert cleared._fast_hits == 0 and not torch.equal(masked[-1], want[-1])
    cleared.clear_inpaint()
    for rep in range(4):
        got = run(cleared, x, outs)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (rep, i)
    assert never._fast_hits == 0
    assert cleared._fast_hits >= 2 * (STEPS - 2), cleared._fast_hits  # the fast path serves the later runs again


def test_masked_steps_in_a_captured_graph(dev):
    "three masked Euler steps captured on one stream (no parallel branches), replayed once: the eager run's bits"
    make = lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled()))  # noqa: E731
    x, orig, nz, outs, mask = inpaint_inputs(dev, 25)

    def three_steps(w):
        w.set_timesteps(STEPS)
        y = x
        for i, t in enumerate(w.timesteps.tolist()[:3]):
            y = w.step(outs[i], t, y, return_dict=False)[0]
        return y

    eager = make()
    eager.set_inpaint(mask, orig, nz)
    want = three_steps(eager).clone()
    captured = make()
    captured.set_inpaint(mask, orig, nz)
    three_steps(captured)  # (warm-up: the library and the allocator have seen these shapes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = three_steps(captured)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
