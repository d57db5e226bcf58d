"""Guided steps (classifier-free guidance fused into the step launch) on the device.

The contract is one sentence: a guided step returns the bits of the pipeline's three torch lines followed by today's step.  So the
reference of the raw entry is torch's own device ops, live -- p_ref = uncond + g * (cond - uncond) -- and skr_step_launch over the
operand list with p_ref in `slot`; the reference of the wrapper is a twin wrapper stepping with the three lines and step().  Every
comparison is made on integer views of the bits; there is no tolerance anywhere in this file.

Inputs are seeded normal values; fp16 also runs a set scaled by 1e-4 (results in the subnormal range) and one scaled by 4000 (g * d
overflows to inf).  No NaN inputs.  Scales: 7.5 (exact in bf16), 7.3 and 3.3 (which tell an fp32 scalar from one rounded to the tensor
dtype), 1.0 and 0.0."""

import ctypes
import itertools

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu

OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
SCALES = (7.5, 7.3, 3.3, 1.0, 0.0)
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
COUNTS = (1, 2, 4, 5, 8, 9, 12, 13, 16)  # both sides of every kernarg slot size


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def same_bits(a, b):
    a, b = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype]))


def differing(a, b):
    "how many elements differ in their bits, and the first few pairs: what a failing comparison prints"
    a, b = a.contiguous().view(INT_VIEW[a.dtype]).flatten(), b.contiguous().view(INT_VIEW[b.dtype]).flatten()
    at = (a != b).nonzero().flatten()
    return int(at.numel()), a.numel(), [(int(i), hex(int(a[i]) & 0xFFFFFFFF), hex(int(b[i]) & 0xFFFFFFFF)) for i in at[:4]]


def normal(shape, dtype, dev, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(dev)


def make_plan(n, dtype, draw, sample_numel, n_a=None, dtype_b=None, out_dtype=None, acc_f64=False):
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a = n, n if n_a is None else n_a
    plan.dtype_a = _hip.DTYPE_CODE[dtype]
    plan.dtype_b = _hip.DTYPE_CODE[dtype_b if dtype_b is not None else torch.float32]
    plan.out0_dtype, plan.out1_dtype = _hip.DTYPE_CODE[out_dtype if out_dtype is not None else dtype], _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k in range(n):
        plan.coef0[k] = (-1.0) ** k * (0.3 + 0.17 * k)
    if draw:
        plan.noise_mode, plan.zeta0, plan.stream0, plan.sample_numel = 1, 0.45, 512, sample_numel
    return plan


def launch_guided(plan, inputs, out, cond, guided_out, scale, slot, seeds, dev):
    _hip.launch_step_guided(plan, inputs, out, cond, guided_out, scale, slot, seeds, inputs[0].numel(), dev)


def check_case(dev, shape, dtypes, slot, draw, store, scale, seed, dtype_out=None, acc_f64=False, value_scale=1.0, n_a=None):
    """one launch of the raw entry against torch's three device ops and skr_step_launch; `dtypes`: one dtype per operand (grouped)"""
    n = len(dtypes)
    inputs = [normal(shape, dtypes[k], dev, seed + k, value_scale) for k in range(n)]
    cond = normal(shape, dtypes[slot], dev, seed + 100, value_scale)
    seeds = torch.tensor([11, 22, 33, 44][: shape[0]], dtype=torch.int64, device=dev)
    numel = inputs[0].numel()
    group_b = next((d for d in dtypes if d != dtypes[0]), None)
    plan = make_plan(n, dtypes[0], draw, numel // shape[0], n_a=n_a if n_a is not None else sum(1 for d in dtypes if d == dtypes[0]),
                     dtype_b=group_b if group_b is not None else (torch.float64 if acc_f64 else torch.float32), out_dtype=dtype_out, acc_f64=acc_f64)  # fmt: skip
    out_dtype = dtype_out if dtype_out is not None else dtypes[0]
    uncond = inputs[slot]
    p_ref = uncond + scale * (cond - uncond)
    assert p_ref.dtype == uncond.dtype
    want = torch.zeros(shape, dtype=out_dtype, device=dev)
    _hip.launch_step(plan, inputs[:slot] + [p_ref] + inputs[slot + 1 :], want, None, seeds if draw else None, numel, dev)
    got = torch.zeros(shape, dtype=out_dtype, device=dev)
    guided = torch.zeros_like(uncond) if store else None
    launch_guided(plan, inputs, got, cond, guided, scale, slot, seeds if draw else None, dev)
    what = (tuple(shape), [str(d) for d in dtypes], slot, draw, store, scale)
    if store:
        assert same_bits(guided, p_ref), (what, differing(guided, p_ref))
    assert same_bits(got, want), (what, differing(got, want))
    return got, guided


def slots_of(n):
    return sorted({0, n // 2, n - 1})


# the shapes of the grid: the one-trip kernel's (2 samples of 2048 elements) and the general kernel's (ragged, samples below a chunk,
# 8 elements); (shape, the draws it runs with)
GRID_SHAPES = {"one_trip": ((2, 2048), (False, True)), "ragged_draw": ((2, 4, 10, 10), (True,)), "ragged": ((2, 3, 10, 10), (False,)), "eight": ((1, 8), (False, True))}


@pytest.mark.parametrize("kind", sorted(GRID_SHAPES))
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_raw_entry_equals_torch_plus_step_launch(name, n, kind, dev):
    """the grid: dtype x operand count x slot first / middle / last x with and without a draw x with and without guided_out, on the
    one-trip shape and the general kernel's shapes; the scales rotate through the cases.

    fp16 on the three general-kernel shapes with the scales 7.3 and 3.3 is where torch's OWN `g * d` is not one function of its inputs
    (narrowed with test_guidance_only_form_against_torch_one_op_at_a_time).  Elements in the whole blocks of its vectorised elementwise
    kernel are rounded twice (fp32 product, then fp16), while elements in the last, partial block of that kernel (all 600 here; index
    >= 2048 of a 3000-element tensor) are rounded ONCE from the exact product (a fused multiply-and-convert in torch's scalar tail
    path): 7.3f * 0.1416015625 lies 2.7e-8 above an fp16 tie, its fp32 rounding falls on the tie, and the two roundings give 0x3c22
    where the single one gives 0x3c23.  A kernel that rounds twice everywhere had 1 to 15 of 600 elements off by one fp16 ulp here; the
    general kernel therefore rounds once from the last multiple of 2048 on, as torch does.  bf16, fp32 and fp64 have no such fused
    instruction."""
    dtype = DTYPES[name]
    shape, draws = GRID_SHAPES[kind]
    scales = itertools.cycle(SCALES)
    for slot, draw, store in itertools.product(slots_of(n), draws, (False, True)):
        check_case(dev, shape, [dtype] * n, slot, draw, store, next(scales), seed=1000 * n + slot)
        check_case(dev, shape, [dtype] * n, slot, draw, store, next(scales), seed=2000 * n + slot)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_the_two_kernels_agree_bit_for_bit(name, dev):
    "a subset of the grid again with one_trip 0: the general kernel on the one-trip shape gives the one-trip kernel's bits (and torch's)"
    lib, dtype = _hip.load(), DTYPES[name]
    for n, draw in itertools.product((1, 4, 5, 16), (False, True)):
        slot = n // 2
        a, pa = check_case(dev, (2, 2048), [dtype] * n, slot, draw, True, 7.3, seed=50 * n)
        assert lib.skr_set_tuning(b"one_trip", 0) == 0
        try:
            b, pb = check_case(dev, (2, 2048), [dtype] * n, slot, draw, True, 7.3, seed=50 * n)
        finally:
            lib.skr_set_tuning(b"one_trip", 1)
        assert same_bits(a, b) and same_bits(pa, pb), (n, draw)


@pytest.mark.parametrize("shape", [(2, 2048), (2, 3, 10, 10)], ids=["one_trip", "ragged"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name,value_scale", [("bf16", 1.0), ("fp16", 1.0), ("fp16", 1e-4), ("fp16", 4000.0), ("fp32", 1.0)])
def test_every_scale_and_value_range(name, value_scale, scale, shape, dev):
    """all five scales on every value set: the fused launch and the guidance-only form against torch's three ops.
    fp16 on the ragged shape with 7.3 and 3.3 meets torch's partial last block, which rounds g * d once (see the grid's docstring)."""
    dtype = DTYPES[name]
    for shape in (shape,):
        _, guided = check_case(dev, shape, [dtype] * 3, 1, False, True, scale, seed=7, value_scale=value_scale)
        if value_scale == 4000.0 and scale > 7.0:
            assert torch.isinf(guided.float()).any()  # g * d overflowed, as in torch
        if value_scale == 1e-4:
            assert (guided.float().abs() < 2.0**-14).any()  # subnormal results
        u, c = normal(shape, dtype, dev, 8, value_scale), normal(shape, dtype, dev, 108, value_scale)
        assert same_bits(lazy.guide_only(lazy.Guidance(u, c, scale)), u + scale * (c - u))


@pytest.mark.parametrize("shape", [(2, 2048), (3, 1000)], ids=["whole_blocks", "ragged"])
@pytest.mark.parametrize("dtype", [*DTYPES.values(), torch.float64], ids=[*DTYPES, "fp64"])
def test_guidance_only_form_against_torch_one_op_at_a_time(dtype, shape, dev):
    """the narrowing tool: with g = 1 the launch isolates the subtraction and the addition (m = d exactly), with uncond = 0 it
    isolates the multiplication (d = cond, p = m exactly): each of torch's three device ops against the kernel's, per dtype.
    The ragged shape has both of torch's fp16 roundings of the product in one tensor: twice below index 2048, once from there on (see
    the grid's docstring; with two roundings everywhere 7 of the 3000 elements differed, all at index >= 2048)."""
    for dtype in (dtype,):
        u, c = normal(shape, dtype, dev, 31), normal(shape, dtype, dev, 32)
        zero = torch.zeros_like(u)
        for g in (7.3, 3.3):
            got = lazy.guide_only(lazy.Guidance(zero, c, g))
            assert same_bits(got, g * c), (dtype, g, "mul", differing(got, g * c))
        d = c - u
        assert same_bits(lazy.guide_only(lazy.Guidance(zero, d, 1.0)), d)
        got = lazy.guide_only(lazy.Guidance(u, c, 1.0))
        assert same_bits(got, u + d), (dtype, "sub, add", differing(got, u + d))


def test_fp64_tensors_and_fp64_accumulation(dev):
    for n, slot, draw in ((1, 0, False), (3, 1, True), (5, 4, False)):
        check_case(dev, (2, 2048), [torch.float64] * n, slot, draw, True, 7.3, seed=60 + n, acc_f64=True)
        check_case(dev, (2, 3, 10, 10), [torch.float64] * n, slot, False, True, 3.3, seed=70 + n, acc_f64=True)
    # 16-bit tensors under acc_f64: the guidance stays fp32 op-math, p is widened exactly
    for dtype in (torch.bfloat16, torch.float16):
        check_case(dev, (2, 2048), [dtype] * 3, 1, True, True, 7.3, seed=80, acc_f64=True)
        check_case(dev, (2, 2048), [dtype, dtype, torch.float64], 0, False, True, 3.3, seed=81, acc_f64=True, dtype_out=torch.float64)


def test_two_dtype_groups_with_the_slot_in_either(dev):
    "bf16 guidance beside an fp32 sample, and the reverse"
    mixed = [torch.bfloat16, torch.bfloat16, torch.float32]
    for shape, draw in (((2, 2048), True), ((2, 4, 10, 10), True), ((2, 3, 10, 10), False)):
        for slot in (0, 1, 2):
            for out in (torch.bfloat16, torch.float32):
                check_case(dev, shape, mixed, slot, draw, True, 7.3, seed=90 + slot, dtype_out=out)


@pytest.mark.parametrize("dtype", [*DTYPES.values(), torch.float64], ids=[*DTYPES, "fp64"])
def test_guidance_only_form_through_the_raw_entry(dtype, dev):
    "whole blocks of torch's kernel, a tensor below one, and (5000 elements) whole blocks with a partial one behind them"
    for dtype in (dtype,):
        for shape in ((2, 2048), (4, 1024), (7,), (2, 3, 10, 10), (5, 1000)):
            u, c = normal(shape, dtype, dev, 41), normal(shape, dtype, dev, 42)
            plan = _hip.StepPlanC()
            plan.n_terms = plan.n_group_a = 1
            plan.dtype_a = plan.dtype_b = _hip.DTYPE_CODE[dtype]
            plan.out0_dtype = plan.out1_dtype = _hip.NONE
            plan.acc_f64 = 1 if dtype == torch.float64 else 0
            plan.coef0[0] = 1.0
            p = torch.zeros_like(u)
            launch_guided(plan, [u], None, c, p, 7.3, 0, None, dev)
            assert same_bits(p, u + 7.3 * (c - u)), (dtype, shape)


# ---- the status table ------------------------------------------------------------------------------------------------------------
def test_status_table_in_order_and_nothing_written(dev):
    "every check of the entry in its order, two-fault rows for adjacent checks, the outputs still zero afterwards"
    lib = _hip.load()
    numel = 8192
    a, b, cond = (normal((2, 4096), torch.bfloat16, dev, 200 + k) for k in range(3))
    out, gout = torch.zeros_like(a), torch.zeros_like(a)
    seeds = torch.tensor([5, 6], dtype=torch.int64, device=dev)

    def plan_of(**fields):
        plan = make_plan(2, torch.bfloat16, True, 4096)
        for key, value in fields.items():
            setattr(plan, key, value)
        return plan

    def call(plan=None, inputs=(a.data_ptr(), b.data_ptr()), out=out.data_ptr(), cond=cond.data_ptr(), gout=gout.data_ptr(), slot=1, reserved=0, seeds=seeds.data_ptr(),
             numel=numel, no_plan=False, no_guide=False, no_inputs=False):  # fmt: skip
        plan = plan if plan is not None else plan_of()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
        return lib.skr_step_launch_guided(None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide), seeds, numel, None)

    only = dict(plan=plan_of(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a.data_ptr(),), slot=0)
    table = [
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("a draw without seeds", dict(seeds=None), NULL),
        ("too many operands", dict(plan=plan_of(n_terms=17, n_group_a=17)), TERMS),
        ("group a beyond the operands", dict(plan=plan_of(n_group_a=3)), TERMS),
        ("slot below the operands", dict(slot=-1), TERMS),
        ("slot beyond the operands", dict(slot=2), TERMS),
        ("negative numel", dict(numel=-8), SHAPE),
        ("no output at all", dict(only, out=None, gout=None), NULL),
        ("noise_mode 2", dict(plan=plan_of(noise_mode=2)), UNSUPPORTED),
        ("a second output", dict(plan=plan_of(out1_dtype=_hip.BF16)), UNSUPPORTED),
        ("chain", dict(plan=plan_of(chain=0.5)), UNSUPPORTED),
        ("zeta1", dict(plan=plan_of(zeta1=0.5)), UNSUPPORTED),
        ("convert_to", dict(plan=plan_of(convert_to=1)), UNSUPPORTED),
        ("convert_from above 3", dict(plan=plan_of(convert_from=4)), UNSUPPORTED),
        ("reserved", dict(reserved=1), UNSUPPORTED),
        ("guidance-only with two operands", dict(plan=plan_of(out0_dtype=_hip.NONE), out=None), UNSUPPORTED),
        ("guidance-only with an out pointer", dict(only), UNSUPPORTED),
        ("samples that do not divide the launch", dict(plan=plan_of(sample_numel=4095)), SHAPE),
        ("no sample size under a draw", dict(plan=plan_of(sample_numel=0)), SHAPE),
        ("samples of 4 elements under a draw", dict(plan=plan_of(sample_numel=4)), UNSUPPORTED),
        ("empty launch", dict(numel=0, inputs=(None, None), out=None, cond=None), OK),
        ("no inputs", dict(no_inputs=True), NULL),
        ("no out", dict(out=None), NULL),
        ("no cond", dict(cond=None), NULL),
        ("a NULL operand", dict(inputs=(a.data_ptr(), None)), NULL),
        ("a misaligned operand", dict(inputs=(a.data_ptr(), b.data_ptr() + 2)), ALIGN),
        ("a misaligned out", dict(out=out.data_ptr() + 4), ALIGN),
        ("a misaligned cond", dict(cond=cond.data_ptr() + 2), ALIGN),
        ("a misaligned guided_out", dict(gout=gout.data_ptr() + 8), ALIGN),
        ("fp64 operands without acc_f64", dict(plan=plan_of(dtype_a=_hip.F64, out0_dtype=_hip.F64)), DTYPE),
        ("an fp64 group for the slot without acc_f64", dict(plan=plan_of(n_group_a=1, dtype_b=_hip.F64)), DTYPE),
        ("an out dtype outside the groups", dict(plan=plan_of(out0_dtype=_hip.F16)), DTYPE),
        # two faults: the earlier check answers
        ("no seeds + slot", dict(seeds=None, slot=5), NULL),
        ("slot + negative numel", dict(slot=2, numel=-1), TERMS),
        ("negative numel + reserved", dict(numel=-1, reserved=1), SHAPE),
        ("reserved + sample size", dict(reserved=1, plan=plan_of(sample_numel=4095)), UNSUPPORTED),
        ("sample size + no cond", dict(plan=plan_of(sample_numel=4095), cond=None), SHAPE),
        ("no cond + misaligned out", dict(cond=None, out=out.data_ptr() + 4), NULL),
        ("misaligned cond + dtype", dict(cond=cond.data_ptr() + 2, plan=plan_of(out0_dtype=_hip.F16)), ALIGN),
    ]
    for what, kwargs, want in table:
        assert call(**kwargs) == want, what
    torch.cuda.synchronize()
    assert not out.any() and not gout.any()  # no refused launch wrote anything
    # one well-formed control per dtype
    for dtype in (*DTYPES.values(), torch.float64):
        check_case(dev, (2, 2048), [dtype] * 2, 1, True, True, 7.5, seed=300, acc_f64=dtype == torch.float64)


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------------
LATENTS, STEPS = (2, 4, 32, 32), 6
ONE_LAUNCH = {
    "euler": lambda: PT.Euler(),
    "dpm2": lambda: PT.DPM(order=2),
    "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1),
    "adams3": lambda: PT.Adams(order=3),
    "unip2": lambda: PT.UniP(order=2),
}
TWO_LAUNCH = {"unipc2": lambda: PT.UniPC(order=2), "spc": lambda: PT.SPC()}


def network_outputs(dev, dtype, seed):
    "per step: the halves of one doubled-batch output, as chunk(2) views"
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(LATENTS, generator=g).to(dtype).to(dev)
    outs = [torch.randn((2 * LATENTS[0], *LATENTS[1:]), generator=g).to(dtype).to(dev).chunk(2) for _ in range(STEPS)]
    return x, outs


def twins(sampler, dev, launches_per_step, dtype=torch.bfloat16, scale=7.3, guided_at=lambda i: True, prepare=lambda w: None, **fields):
    """twin wrappers: one stepping with step_guided, the other with the three torch lines plus step(); prev_sample and
    pred_original_sample equal in every bit at every step, and the launches of every guided step counted through _hip.trace"""
    make = lambda: PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled()), **fields)  # noqa: E731
    fused, plain = make(), make()
    fused.set_timesteps(STEPS), plain.set_timesteps(STEPS)
    prepare(fused), prepare(plain)
    x, outs = network_outputs(dev, dtype, 77)
    gens = [[torch.Generator().manual_seed(s) for s in (1234, 5678)] for _ in range(2)]
    xa = xb = x
    for i, t in enumerate(plain.timesteps.tolist()):
        uncond, cond = outs[i]
        if guided_at(i):
            _hip.trace = []
            try:
                xa, pa = fused.step_guided(uncond, cond, scale, t, xa, generator=gens[0], return_dict=False)
                launches = len(_hip.trace)
            finally:
                _hip.trace = None
            assert launches_per_step is None or launches == launches_per_step, (i, launches)
        else:
            xa, pa = fused.step(uncond + scale * (cond - uncond), t, xa, generator=gens[0], return_dict=False)
        xb, pb = plain.step(uncond + scale * (cond - uncond), t, xb, generator=gens[1], return_dict=False)
        assert xa.dtype == dtype and same_bits(xa, xb), i
        assert same_bits(pa, pb), i
    assert not fused._programs or not all(guided_at(i) for i in range(STEPS))  # a guided step builds no step program
    return fused, plain


@pytest.mark.parametrize("name", sorted(ONE_LAUNCH))
def test_wrapper_guided_step_is_one_launch(name, dev):
    fused, _ = twins(ONE_LAUNCH[name], dev, 1)
    assert fused._fast_hits == 0 and not fused._fast


@pytest.mark.parametrize("name", sorted(TWO_LAUNCH))
def test_wrapper_two_output_samplers_take_the_guidance_only_launch_first(name, dev):
    twins(TWO_LAUNCH[name], dev, 2)


def test_wrapper_guided_step_under_set_inpaint_is_two_launches(dev):
    g = torch.Generator().manual_seed(5)
    orig, nz = (torch.randn(LATENTS, generator=g).bfloat16().to(dev) for _ in range(2))
    mask = (torch.rand((2, 1, 32, 32), generator=g) < 0.5).to(dev)
    twins(ONE_LAUNCH["dpm2"], dev, 2, prepare=lambda w: w.set_inpaint(mask, orig, nz))


@pytest.mark.parametrize("name", ["euler", "dpm2_sde", "adams3"])
def test_wrapper_invert_prediction_is_a_sign(name, dev):
    twins(ONE_LAUNCH[name], dev, 1, invert_prediction=True)


@pytest.mark.parametrize("name", ["euler", "dpm2", "unipc2"])
def test_wrapper_fp16(name, dev):
    twins({**ONE_LAUNCH, **TWO_LAUNCH}[name], dev, 2 if name in TWO_LAUNCH else 1, dtype=torch.float16, scale=3.3)


@pytest.mark.parametrize("name", ["dpm2", "adams3", "unipc2"])
def test_wrapper_run_that_alternates_step_guided_and_step(name, dev):
    "history stays coherent: the guided steps' records hold the stored prediction, the plain steps' the caller's tensor"
    for first in (0, 1):
        twins({**ONE_LAUNCH, **TWO_LAUNCH}[name], dev, 2 if name in TWO_LAUNCH else 1, guided_at=lambda i, first=first: i % 2 == first)


def test_wrapper_compute_scale_none_and_float64_and_channels_last(dev):
    "what the one launch does not cover keeps the same bits: the op tape, fp64 accumulation (one launch, the general kernel), channels-last"
    twins(ONE_LAUNCH["dpm2"], dev, None, compute_scale=None)  # (the op tape's launch is not a step launch: not counted)
    twins(ONE_LAUNCH["dpm2"], dev, 1, compute_scale=torch.float64)
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))  # noqa: E731
    fused, plain = make(), make()
    fused.set_timesteps(STEPS), plain.set_timesteps(STEPS)
    x, outs = network_outputs(dev, torch.bfloat16, 78)
    xa = xb = x.contiguous(memory_format=torch.channels_last)
    for i, t in enumerate(plain.timesteps.tolist()):
        uncond, cond = (h.contiguous(memory_format=torch.channels_last) for h in outs[i])
        xa, pa = fused.step_guided(uncond, cond, 7.3, t, xa, return_dict=False)
        xb, pb = plain.step(uncond + 7.3 * (cond - uncond), t, xb, return_dict=False)
        assert same_bits(xa, xb) and same_bits(pa, pb) and xa.stride() == xb.stride(), i


def test_wrapper_grad_recorded_cond(dev):
    "a cond that autograd records: torch's three lines (which it records) and the recorded step; the gradient of the unfused run"
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))  # noqa: E731
    x, outs = network_outputs(dev, torch.float32, 79)
    grads, finals = [], []
    for guided in (True, False):
        w = make()
        w.set_timesteps(STEPS)
        conds = [c.clone().requires_grad_() for _, c in outs]
        y = x
        for i, t in enumerate(w.timesteps.tolist()[:3]):
            u, c = outs[i][0], conds[i]
            y = w.step_guided(u, c, 7.3, t, y, return_dict=False)[0] if guided else w.step(u + 7.3 * (c - u), t, y, return_dict=False)[0]
        y.float().square().sum().backward()
        grads.append([c.grad for c in conds[:3]])
        finals.append(y.detach())
    assert same_bits(finals[0], finals[1])
    for ga, gb in zip(*grads):
        assert ga is not None and same_bits(ga, gb)


def test_guided_step_under_the_indexed_hook_raises_with_the_reason(dev):
    w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled()))
    w.set_timesteps(STEPS)
    x, outs = network_outputs(dev, torch.bfloat16, 80)
    _hip.indexed = object()  # (never asked anything: a guided launch refuses before it looks at the hook's table)
    try:
        with pytest.raises(_hip.SkrampleHipError, match="captured loops"):
            w.step_guided(outs[0][0], outs[0][1], 7.5, w.timesteps.tolist()[0], x)
    finally:
        _hip.indexed = None
