"""Guided in-painting on the device: skr_guided_masked_step_launch against today's two launches (bit for bit), against float64 with the
bound of tests/test_masked_gpu.py -- 2 (n + 4) 2^-24 M + u_out |ref| + tiny_out, n operands (+1 with noise), M the sum of the absolute
terms --, its refusals, and SkrampleWrapperScheduler.set_inpaint(fuse_guidance=True) against the default route."""

import ctypes

import numpy as np
import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
U_OUT_TINY = {torch.bfloat16: (2.0**-8, 2.0**-133), torch.float32: (2.0**-24, 2.0**-149)}
ERR_NULL, ERR_TERMS, ERR_ALIGN, ERR_UNSUPPORTED = 1, 3, 4, 7
SHAPES = {  # (latents per sample, mask per sample, batch, one mask for the whole batch)
    "wraps_twice_in_a_chunk": ((4, 32, 32), (1, 32, 32), 3, False),
    "wraps_mid_chunk": ((4, 96, 96), (1, 96, 96), 1, False),  # 18 chunks per sample, the mask wraps every 4.5
    "batch_stride_0": ((4, 64, 64), (1, 64, 64), 3, True),
    "full_mask": ((4, 32, 32), (4, 32, 32), 3, False),
}
SCALES, STREAM, ZETA, dev = (7.5, 7.3, 3.3), 512, 0.45, torch.device("cuda:0")


def same_bits(a, b):
    a, b = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (a, b))  # (pred_original_sample may be lazy)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype]))


class Problem:
    "operands, cond, a soft mask with one row of ones and one of zeros, and coefficients: the last two operands carry coef1"

    def __init__(self, name, dtype, n, seed):
        unit, munit, batch, whole = SHAPES[name]
        self.shape, self.n, g = (batch, *unit), n, torch.Generator().manual_seed(seed)
        *self.ops, self.cond = (torch.randn(self.shape, generator=g).to(dtype).to(dev) for _ in range(n + 1))
        mshape = (1 if whole else batch, *munit)
        mask = torch.rand(mshape, generator=g)
        mask[..., 0, :], mask[..., 1, :] = 1.0, 0.0
        self.mask = mask.to(dtype).to(dev)
        self.mask_numel, self.batch_stride = lazy.mask_layout(mshape, self.shape)
        self.numel, self.seeds = self.cond.numel(), torch.tensor([11, 22, 33][:batch], dtype=torch.int64, device=dev)

    def plan(self, slot, draw):
        n, plan = self.n, _hip.StepPlanC()
        plan.n_terms, plan.n_group_a, plan.dtype_a, plan.out0_dtype = n, n, _hip.DTYPE_CODE[self.cond.dtype], _hip.DTYPE_CODE[self.cond.dtype]
        plan.dtype_b, plan.out1_dtype, plan.sample_numel = _hip.F32, _hip.NONE, self.numel // self.shape[0]
        for k in range(n):  # (the known form never holds the prediction: with 3 operands and the middle slot only the last one carries coef1)
            plan.coef0[k] = (-1.0) ** k * (0.3 + 0.17 * k) if k < n - 1 else 0.0
            plan.coef1[k] = (0.8, -0.35)[k - (n - 2)] if k >= n - 2 and k != slot else 0.0
        plan.noise_mode, plan.zeta0, plan.stream0 = (1, ZETA, STREAM) if draw else (0, 0.0, 0)
        return plan

    def one_launch(self, plan, slot, draw, scale, phi=0.0, factor=None):
        got, guided = torch.zeros_like(self.cond), torch.zeros_like(self.cond)
        _hip.launch_guided_masked_step(plan, self.ops, got, self.cond, guided, scale, slot, self.mask, self.mask_numel, self.batch_stride, self.seeds if draw else None, self.numel, dev, factor, phi)
        return got, guided


@pytest.mark.parametrize("n", [3, 5, 9, 16])  # both sides of the kernarg slot sizes
@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_the_entry_equals_the_two_launches_bit_for_bit(dtype, name, n):
    pr = Problem(name, dtype, n, seed=100 + n)
    cases = [(slot, draw, phi) for slot in (0, n // 2) for draw in (False, True) for phi in (0.0, 0.7)]
    for case, (slot, draw, phi) in enumerate(cases):
        scale, plan, u = SCALES[case % 3], pr.plan(slot, draw), pr.ops[slot]
        guidance = lazy.Guidance(u, pr.cond, scale, phi)  # today's route: the guidance-only launch, then the masked step with p in `slot`
        p_ref, want = lazy.guide_only(guidance), torch.zeros_like(pr.cond)
        _hip.launch_step_masked(plan, pr.ops[:slot] + [p_ref] + pr.ops[slot + 1 :], want, pr.mask, pr.mask_numel, pr.batch_stride, pr.seeds if draw else None, pr.numel, dev)
        got, guided = pr.one_launch(plan, slot, draw, scale, phi, guidance.device_factor(u, pr.cond) if phi else None)
        assert same_bits(guided, p_ref) and same_bits(got, want), (str(dtype), name, n, slot, draw, phi, scale)


@pytest.mark.parametrize("name", ["wraps_twice_in_a_chunk", "wraps_mid_chunk"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_against_float64(dtype, name):
    n, slot, pr = 5, 2, Problem(name, dtype, 5, seed=7)
    got, guided = pr.one_launch(plan := pr.plan(slot, True), slot, True, 7.3)
    f64 = lambda t: t.cpu().double().numpy()  # noqa: E731
    z = f64(lazy.PhiloxNoise(pr.seeds, STREAM, pr.shape, dev).realize(torch.float32))
    v = [f64(guided) if k == slot else f64(pr.ops[k]) for k in range(n)]
    m = np.broadcast_to(f64(pr.mask).reshape((-1, *SHAPES[name][1])), pr.shape)
    ref = m * (sum(plan.coef0[k] * v[k] for k in range(n)) + ZETA * z) + (1 - m) * sum(plan.coef1[k] * v[k] for k in range(n))
    magnitude = np.abs(m) * (sum(abs(plan.coef0[k] * v[k]) for k in range(n)) + ZETA * np.abs(z)) + np.abs(1 - m) * sum(abs(plan.coef1[k] * v[k]) for k in range(n))
    bound = 2 * (n + 1 + 4) * 2.0**-24 * magnitude + U_OUT_TINY[dtype][0] * np.abs(ref) + U_OUT_TINY[dtype][1]
    worst = float((np.abs(f64(got) - ref) / bound).max())
    print(f"guided masked {dtype} {name}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


REFUSALS = {  # what is changed in a launch the entry takes: (plan, guide, mask, arguments)
    "coef1_of_the_slot": (ERR_UNSUPPORTED, lambda p, g, m, a: setattr(p, "coef1", type(p.coef1)(0.0, 0.5))),
    "numel_not_whole_chunks": (ERR_UNSUPPORTED, lambda p, g, m, a: (setattr(p, "sample_numel", 3072), a.update(numel=3072))),
    "sample_of_1024": (ERR_UNSUPPORTED, lambda p, g, m, a: setattr(p, "sample_numel", 1024)),
    "mask_of_another_dtype": (ERR_UNSUPPORTED, lambda p, g, m, a: setattr(m, "dtype", _hip.F32)),
    "acc_f64": (ERR_UNSUPPORTED, lambda p, g, m, a: setattr(p, "acc_f64", 1)),
    "no_step_output": (ERR_UNSUPPORTED, lambda p, g, m, a: setattr(p, "out0_dtype", _hip.NONE)),
    "null_guide": (ERR_NULL, lambda p, g, m, a: a.update(guide=None)),
    "null_mask": (ERR_NULL, lambda p, g, m, a: a.update(mask=None)),
    "null_cond": (ERR_NULL, lambda p, g, m, a: setattr(g, "cond", None)),
    "misaligned_cond": (ERR_ALIGN, lambda p, g, m, a: setattr(g, "cond", g.cond + 2)),
    "slot_out_of_range": (ERR_TERMS, lambda p, g, m, a: setattr(g, "slot", 3)),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_write_nothing(name):
    plan = (pr := Problem("wraps_twice_in_a_chunk", torch.bfloat16, 3, seed=3)).plan(1, False)
    out, guided = (torch.full(pr.shape, 123.0, dtype=torch.bfloat16, device=dev) for _ in range(2))
    guide = _hip.StepGuidanceC(pr.cond.data_ptr(), guided.data_ptr(), 7.3, 1, 0)
    mask = _hip.StepMaskC(pr.mask.data_ptr(), _hip.BF16, 0, pr.mask_numel, pr.batch_stride)
    args = {"numel": pr.numel, "guide": ctypes.byref(guide), "mask": ctypes.byref(mask)}
    REFUSALS[name][1](plan, guide, mask, args)
    arr = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in pr.ops])
    status = _hip.load().skr_guided_masked_step_launch(ctypes.byref(plan), arr, out.data_ptr(), args["guide"], None, args["mask"], None, args["numel"], _hip.current_stream_ptr(dev))
    assert status == REFUSALS[name][0]
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and bool((guided == 123.0).all())


LATENTS, STEPS, SCALE = (2, 4, 32, 32), 5, 7.3
SAMPLERS = {"euler": PT.Euler, "dpm2": lambda: PT.DPM(order=2), "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1), "adams3": lambda: PT.Adams(order=3),
            "unip2": lambda: PT.UniP(order=2), "unipc2": lambda: PT.UniPC(order=2)}  # fmt: skip


def lines(u, c, phi):  # the pipeline's lines, with the factor of Guidance.factor() where torch would take its own two stds
    p = u + SCALE * (c - u)
    return p if phi == 0.0 else phi * (p * lazy.Guidance(u, c, SCALE).factor()) + (1 - phi) * p


def traced(call):
    _hip.trace = []
    try:
        return call(), [e.kind for e in _hip.trace]
    finally:
        _hip.trace = None


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_wrapper_twins(name, phi):
    "set_inpaint(fuse_guidance=True) + step_guided, set_inpaint + step_guided (the default route), set_inpaint + torch's lines + step(): the same bits"
    g = torch.Generator().manual_seed(5)
    orig, nz, x = (torch.randn(LATENTS, generator=g).bfloat16().to(dev) for _ in range(3))
    mask = torch.rand((2, 1, 32, 32), generator=g).to(dev)
    outs = [torch.randn((4, *LATENTS[1:]), generator=g).bfloat16().to(dev).chunk(2) for _ in range(STEPS)]
    fused, default, plain = (PD.SkrampleWrapperScheduler(SAMPLERS[name](), PS.Karras(PS.Scaled())) for _ in range(3))
    fused.set_timesteps(STEPS), default.set_timesteps(STEPS), plain.set_timesteps(STEPS)
    fused.set_inpaint(mask, orig, nz, fuse_guidance=True), default.set_inpaint(mask, orig, nz), plain.set_inpaint(mask, orig, nz)
    gens, xa, xb, xc = [[torch.Generator().manual_seed(s) for s in (1234, 5678)] for _ in range(3)], x, x, x
    for i, (t, (u, c)) in enumerate(zip(plain.timesteps.tolist(), outs)):
        (xa, pa), kinds = traced(lambda: fused.step_guided(u, c, SCALE, t, xa, generator=gens[0], return_dict=False, guidance_rescale=phi))
        (xb, pb), usual = traced(lambda: default.step_guided(u, c, SCALE, t, xb, generator=gens[1], return_dict=False, guidance_rescale=phi))
        xc, pc = plain.step(lines(u, c, phi), t, xc, generator=gens[2], return_dict=False)
        assert same_bits(xa, xc) and same_bits(xb, xc) and same_bits(pa, pc) and same_bits(pb, pc), i
        # one launch, behind the statistics launch when rescaled, where the default route takes one more; UniPC (two outputs): the flag changes nothing
        want = usual if name == "unipc2" else (["guidance_factor"] if phi else []) + ["guided_masked"]
        assert kinds == want and (name == "unipc2" or len(usual) == len(kinds) + 1), (i, kinds, usual)
    fused.clear_inpaint(), fused.set_timesteps(STEPS)  # the flag is forgotten: a guided step is one plain guided launch again
    _, kinds = traced(lambda: fused.step_guided(*outs[0], SCALE, fused.timesteps.tolist()[0], x, generator=gens[0], return_dict=False))
    assert not fused._inpaint_fuse and (name == "unipc2" or kinds == ["guided"]), kinds
