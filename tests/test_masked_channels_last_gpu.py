"""Masked (in-painting) steps on channels-last operands, on the device.

C ABI: skr_step_launch_masked_channels_last over channels-last copies of logical tensors and a mask in logical order gives, viewed
logically, the bits skr_step_launch_masked gives over their contiguous copies and the same mask -- the draw included.  Every comparison
in this module is bitwise (torch.equal compares logical elements whatever the strides): the yardstick is the existing contiguous
launch, so no tolerance is involved.  The one-trip kernel and the general kernel are both run on every one-trip case ("one_trip" 0
forces the general one); skr_stat tells which of them a launch took.

Wrapper level: step() under set_inpaint on channels-last latents runs in place -- one launch on the caller's own tensors, a
channels-last result, no copy -- and equals the contiguous run; mixed layouts, `lazy.channels_last = False` and grad-recorded steps run
the path they ran before."""

import ctypes
import math

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _switches_restored():
    yield
    lazy.channels_last = True
    if torch.cuda.is_available():
        _hip.load().skr_set_tuning(b"one_trip", 1)


def fmt(shape):
    return torch.channels_last if len(shape) == 4 else torch.channels_last_3d


def to_cl(t):
    return t.contiguous(memory_format=fmt(t.shape))


def is_cl(t):
    return t.is_contiguous(memory_format=fmt(t.shape))


def stats():
    lib = _hip.load()
    return lib.skr_stat(b"masked_channels_last_one_trip"), lib.skr_stat(b"masked_channels_last_general")


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def make_plan(n, n_a, dtype_a, out, sample_numel, zeta0=0.0, acc_f64=False):
    "operand k: coef0 never zero; coef1 exactly zero for k % 3 == 1 (an operand absent from the known form)"
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a = n, n_a
    plan.dtype_a, plan.dtype_b = _hip.DTYPE_CODE[dtype_a], _hip.F64 if acc_f64 else _hip.F32
    plan.out0_dtype, plan.out1_dtype = _hip.DTYPE_CODE[out], _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k in range(n):
        plan.coef0[k] = (-1.0) ** k * (0.75 + 0.125 * k)
        plan.coef1[k] = 0.0 if k % 3 == 1 else (0.3 - 0.21 * k)
    plan.zeta0, plan.stream0 = zeta0, 3 * 256
    plan.noise_mode = 1 if zeta0 != 0.0 else 0
    plan.sample_numel = sample_numel
    return plan


def launch(plan, operands, out, mask, mask_numel, batch_stride, seeds, layout=None):
    lib = _hip.load()
    arr = (ctypes.c_void_p * max(len(operands), 1))(*[t.data_ptr() for t in operands])
    desc = _hip.StepMaskC(mask.data_ptr(), _hip.DTYPE_CODE[mask.dtype], 0, mask_numel, batch_stride)
    stream = _hip.current_stream_ptr(out.device)
    if layout is None:
        status = lib.skr_step_launch_masked(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), seeds.data_ptr(), out.numel(), stream)
    else:
        status = lib.skr_step_launch_masked_channels_last(
            ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), seeds.data_ptr(), ctypes.byref(_hip.StepLayoutC(*layout)), out.numel(), stream
        )
    assert status == 0, status
    torch.cuda.synchronize()


def operands_of(shape, dtypes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g).to(dt).to(dev) for dt in dtypes]


def mask_of(mask_shape, dtype, dev, seed):
    "exact 0, exact 1 and soft values in between"
    m = torch.rand(mask_shape, generator=torch.Generator().manual_seed(seed))
    m[m < 0.3], m[m > 0.7] = 0.0, 1.0
    assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
    return m.to(dtype).to(dev).contiguous()


def compare(plan, shape, operands, out_dtype, mask, dev, expect):
    """the contiguous launch against the channels-last launch of the same plan and mask; `expect`: "one_trip" or "general" (which of
    the two kernels runs, by skr_stat).  Returns the contiguous result."""
    mask_numel, batch_stride = lazy.mask_layout(mask.shape, shape)
    seeds = torch.tensor([11 + 2**33 * b for b in range(shape[0])], dtype=torch.int64, device=dev)
    layout = (shape[1], math.prod(shape[2:]))
    want = torch.full(shape, float("nan"), dtype=out_dtype, device=dev)
    launch(plan, operands, want, mask, mask_numel, batch_stride, seeds)
    got = to_cl(torch.full(shape, float("nan"), dtype=out_dtype, device=dev))
    before = stats()
    launch(plan, [to_cl(t) for t in operands], got, mask, mask_numel, batch_stride, seeds, layout)
    after = stats()
    assert (after[0] - before[0], after[1] - before[1]) == {"one_trip": (1, 0), "general": (0, 1)}[expect], (expect, before, after)
    assert is_cl(got) and not torch.isnan(want.float()).any()
    assert torch.equal(got, want), (shape, tuple(mask.shape), float((got.double() - want.double()).abs().max()))
    return want


def both_kernels(plan, shape, operands, dtype, mask, dev):
    lib = _hip.load()
    lib.skr_set_tuning(b"one_trip", 1)
    first = compare(plan, shape, operands, dtype, mask, dev, "one_trip")
    lib.skr_set_tuning(b"one_trip", 0)
    second = compare(plan, shape, operands, dtype, mask, dev, "general")
    lib.skr_set_tuning(b"one_trip", 1)
    assert torch.equal(first, second)
    return first


def one_trip_case(shape, mask_shape, dtype, n, dev):
    "with and without a draw, on both kernels; the draw is not vacuous"
    sample_numel = math.prod(shape[1:])
    assert sample_numel % 2048 == 0
    operands = operands_of(shape, [dtype] * n, dev, 100 + n)
    mask = mask_of(mask_shape, dtype, dev, 200 + n)
    drawn = both_kernels(make_plan(n, n, dtype, dtype, sample_numel, zeta0=0.625), shape, operands, dtype, mask, dev)
    quiet = both_kernels(make_plan(n, n, dtype, dtype, sample_numel), shape, operands, dtype, mask, dev)
    assert not torch.equal(drawn, quiet)


# (shape, C, plane, chunks per sample)
ONE_TRIP_SHAPES = [(3, 4, 16, 64), (2, 8, 16, 32), (2, 16, 8, 32)]


@pytest.mark.parametrize("shape", ONE_TRIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_trip_cases_equal_the_contiguous_launch_bitwise_on_both_kernels(shape, dtype, dev):
    "two chunks per sample; a mask per sample, one mask for the batch, and a (W,) mask that wraps inside the plane"
    assert math.prod(shape[1:]) == 4096
    b, _, h, w = shape
    for n in (1, 2, 5, 8):
        for mask_shape in ((b, 1, h, w), (1, 1, h, w), (w,)):
            one_trip_case(shape, mask_shape, dtype, n, dev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_trip_on_5d_latents(dtype, dev):
    for n in (2, 5):
        one_trip_case((2, 4, 2, 16, 32), (2, 1, 1, 16, 32), dtype, n, dev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_trip_with_a_permuting_chunk_map(dtype, dev):
    "16 samples of one chunk each: 16 chunks is a whole group of 8 runs of 2, so the XCD chunk map moves chunks"
    for n in (1, 5):
        one_trip_case((16, 4, 16, 32), (16, 1, 16, 32), dtype, n, dev)


def test_general_fp32(dev):
    shape = (2, 4, 16, 32)
    operands = operands_of(shape, [torch.float32] * 3, dev, 7)
    mask = mask_of((2, 1, 16, 32), torch.float32, dev, 8)
    compare(make_plan(3, 3, torch.float32, torch.float32, 2048, zeta0=-1.25), shape, operands, torch.float32, mask, dev, "general")


def test_general_odd_channel_count_and_ragged_plane(dev):
    shape = (2, 3, 5, 7)
    operands = operands_of(shape, [torch.bfloat16] * 2, dev, 9)
    mask = mask_of((2, 1, 5, 7), torch.bfloat16, dev, 10)
    compare(make_plan(2, 2, torch.bfloat16, torch.bfloat16, 105), shape, operands, torch.bfloat16, mask, dev, "general")


def test_general_full_size_logical_mask_with_a_draw(dev):
    shape = (2, 4, 16, 32)
    operands = operands_of(shape, [torch.bfloat16] * 3, dev, 11)
    mask = mask_of(shape, torch.bfloat16, dev, 12)
    drawn = compare(make_plan(3, 3, torch.bfloat16, torch.bfloat16, 2048, zeta0=0.5), shape, operands, torch.bfloat16, mask, dev, "general")
    quiet = compare(make_plan(3, 3, torch.bfloat16, torch.bfloat16, 2048), shape, operands, torch.bfloat16, mask, dev, "general")
    assert not torch.equal(drawn, quiet)


def test_general_odd_mask_numel(dev):
    shape = (2, 3, 5, 7)
    operands = operands_of(shape, [torch.bfloat16] * 3, dev, 13)
    mask = mask_of((7,), torch.bfloat16, dev, 14)
    compare(make_plan(3, 3, torch.bfloat16, torch.bfloat16, 105), shape, operands, torch.bfloat16, mask, dev, "general")


def test_general_two_dtype_groups(dev):
    shape = (2, 4, 16, 32)
    operands = operands_of(shape, [torch.bfloat16] * 2 + [torch.float32] * 2, dev, 15)
    mask = mask_of((2, 1, 16, 32), torch.bfloat16, dev, 16)
    compare(make_plan(4, 2, torch.bfloat16, torch.bfloat16, 2048, zeta0=0.75), shape, operands, torch.bfloat16, mask, dev, "general")


def test_general_fp64_arithmetic(dev):
    shape = (2, 4, 16, 32)
    operands = operands_of(shape, [torch.bfloat16] * 2 + [torch.float64], dev, 17)
    mask = mask_of((1, 1, 16, 32), torch.float64, dev, 18)
    compare(make_plan(3, 2, torch.bfloat16, torch.float64, 2048, zeta0=0.5, acc_f64=True), shape, operands, torch.float64, mask, dev, "general")


def test_general_fp32_mask_over_bf16_operands(dev):
    shape = (2, 4, 16, 64)
    operands = operands_of(shape, [torch.bfloat16] * 3, dev, 19)
    mask = mask_of((2, 1, 16, 64), torch.float32, dev, 20)
    compare(make_plan(3, 3, torch.bfloat16, torch.bfloat16, 4096, zeta0=0.5), shape, operands, torch.bfloat16, mask, dev, "general")


def test_one_channel_or_one_position_is_the_contiguous_launch_itself(dev):
    "l(p) = p: neither of the two kernels runs"
    for shape, mask_shape in (((2, 1, 32, 64), (2, 1, 32, 64)), ((2, 2048, 1, 1), (2048, 1, 1))):
        sample_numel = math.prod(shape[1:])
        operands = operands_of(shape, [torch.bfloat16] * 2, dev, 21)
        mask = mask_of(mask_shape, torch.bfloat16, dev, 22)
        mask_numel, batch_stride = lazy.mask_layout(mask.shape, shape)
        seeds = torch.tensor([3, 4], dtype=torch.int64, device=dev)
        plan = make_plan(2, 2, torch.bfloat16, torch.bfloat16, sample_numel, zeta0=0.5)
        want, got = torch.empty(shape, dtype=torch.bfloat16, device=dev), torch.empty(shape, dtype=torch.bfloat16, device=dev)
        launch(plan, operands, want, mask, mask_numel, batch_stride, seeds)
        before = stats()
        launch(plan, operands, got, mask, mask_numel, batch_stride, seeds, (shape[1], math.prod(shape[2:])))
        assert stats() == before and torch.equal(got, want)


# ---- the scheduler wrapper -----------------------------------------------------------------------------------------------------------
SHAPE, STEPS, SEEDS = (2, 4, 32, 32), 6, [1234, 2**40 + 5]
WRAPPERS = {
    # (alias_history=True: the history is the caller's own tensors from the first step on, so no snapshot is ever cloned)
    "euler": lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled()),
    "dpm2_eta1": lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), alias_history=True),
    "unipc2": lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=2), PS.Scaled(), alias_history=True),
}


def wrapper_inputs(dev, seed=41):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(SHAPE, generator=g).bfloat16().to(dev)
    outs = [torch.randn(SHAPE, generator=g).bfloat16().to(dev) for _ in range(STEPS)]
    orig, nz = (torch.randn(SHAPE, generator=g).bfloat16().to(dev) for _ in range(2))
    mask = torch.rand((SHAPE[0], 1, *SHAPE[2:]), generator=g)
    mask[mask < 0.3], mask[mask > 0.7] = 0.0, 1.0
    return x0, outs, orig, nz, mask.to(dev)


def run(w, x0, outs, traced=False):
    "[(prev_sample, trace entries)] of one loop; traced: every step under a `_hip.trace` list"
    w.set_timesteps(len(outs))
    x, traj = x0, []
    for i, t in enumerate(w.timesteps.tolist()):
        entries = None
        if traced:
            _hip.trace = []
        try:
            x = w.step(outs[i], t, x, generator=SEEDS, return_dict=False)[0]
            entries = _hip.trace
        finally:
            _hip.trace = None
        traj.append((x, entries))
    torch.cuda.synchronize()
    return traj


def inpaint_run(name, x0, outs, orig, nz, mask, traced=False):
    w = WRAPPERS[name]()
    w.set_inpaint(mask, orig, nz)
    return w, run(w, x0, outs, traced)


@pytest.mark.parametrize("name", ["dpm2_eta1", "euler"])
def test_inpainting_steps_run_in_place_on_channels_last_latents(name, dev):
    "one launch per step on the caller's own tensors and earlier outputs, a channels-last result, the contiguous run's bits"
    x0, outs, orig, nz, mask = wrapper_inputs(dev)
    _, want = inpaint_run(name, x0, outs, orig, nz, mask)
    x0_cl, outs_cl, orig_cl, nz_cl = to_cl(x0), [to_cl(o) for o in outs], to_cl(orig), to_cl(nz)
    before = stats()
    w, got = inpaint_run(name, x0_cl, outs_cl, orig_cl, nz_cl, mask, traced=True)
    assert stats() == (before[0] + STEPS, before[1])  # bf16, C = 4, two chunks per sample: the one-trip kernel, every step
    known = {t.data_ptr() for t in (x0_cl, orig_cl, nz_cl, *outs_cl)}
    for i, ((a, entries), (b, _)) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and torch.equal(a, b), (name, i)
        assert is_cl(a) and b.is_contiguous(), (name, i)
        assert len(entries) == 1 and entries[0].kind == "masked", (name, i, len(entries))  # exactly one launch, the masked one
        (plan, operands, out, _, _, _), used_mask = entries[0], entries[0].mask
        for t in operands:  # the caller's tensors, or what an earlier step of this loop wrote: no copy has been made
            assert t.data_ptr() in known and lazy.layout_of(t) == (4, 1024), (name, i)
        assert used_mask.data_ptr() == w._inpaint[0].data_ptr() and used_mask.is_contiguous(), (name, i)  # the wrapper's own, in logical order
        assert out.data_ptr() == a.data_ptr() and lazy.layout_of(out) == (4, 1024), (name, i)
        known.add(out.data_ptr())


def test_unipc_makes_two_launches_per_step_both_in_place(dev):
    x0, outs, orig, nz, mask = wrapper_inputs(dev, 42)
    _, want = inpaint_run("unipc2", x0, outs, orig, nz, mask)
    x0_cl, outs_cl, orig_cl, nz_cl = to_cl(x0), [to_cl(o) for o in outs], to_cl(orig), to_cl(nz)
    before = stats()
    _, got = inpaint_run("unipc2", x0_cl, outs_cl, orig_cl, nz_cl, mask, traced=True)
    assert sum(stats()) == sum(before) + STEPS  # every blend launch is a channels-last one
    known = {t.data_ptr() for t in (x0_cl, orig_cl, nz_cl, *outs_cl)}
    for i, ((a, entries), (b, _)) in enumerate(zip(got, want)):
        assert torch.equal(a, b) and is_cl(a) and b.is_contiguous(), i
        assert [e.kind for e in entries] == ["plain", "masked"], (i, [e.kind for e in entries])  # the step launch, then the identity-form blend
        for entry in entries:
            for t in entry[1]:
                assert t.data_ptr() in known and lazy.layout_of(t) == (4, 1024), i
            for o in entry[2:4]:
                if o is not None:
                    assert lazy.layout_of(o) == (4, 1024), i
                    known.add(o.data_ptr())


def test_a_contiguous_original_among_channels_last_latents_returns_the_contiguous_result(dev):
    x0, outs, orig, nz, mask = wrapper_inputs(dev, 43)
    _, want = inpaint_run("dpm2_eta1", x0, outs, orig, nz, mask)
    before = stats()
    _, got = inpaint_run("dpm2_eta1", to_cl(x0), [to_cl(o) for o in outs], orig, to_cl(nz), mask)  # a mixed layout: the path it took before
    assert stats() == before
    for i, ((a, _), (b, _)) in enumerate(zip(got, want)):
        assert torch.equal(a, b) and a.is_contiguous(), i


def test_the_switch_restores_the_copying_path(dev):
    x0, outs, orig, nz, mask = wrapper_inputs(dev, 44)
    _, want = inpaint_run("dpm2_eta1", x0, outs, orig, nz, mask)
    lazy.channels_last = False
    before = stats()
    _, got = inpaint_run("dpm2_eta1", to_cl(x0), [to_cl(o) for o in outs], to_cl(orig), to_cl(nz), mask)
    assert stats() == before  # no masked channels-last launch
    for i, ((a, _), (b, _)) in enumerate(zip(got, want)):
        assert torch.equal(a, b) and a.is_contiguous(), i


def test_a_grad_recorded_masked_step_takes_the_old_path_and_backpropagates(dev):
    x0, outs, orig, nz, mask = wrapper_inputs(dev, 45)
    mask = mask.bfloat16()
    results = []
    for conv in ((lambda t: t), to_cl):
        x = conv(x0).detach().requires_grad_()
        form = lazy.lift(x) * 1.25 + lazy.lift(conv(outs[0])) * -0.75
        known = lazy.lift(conv(orig)) * 0.9 + lazy.lift(conv(nz)) * 0.45
        before = stats()
        out = lazy.evaluate_masked(form, known, mask, dtype=torch.bfloat16)
        assert stats() == before and out.requires_grad
        out.float().sum().backward()
        results.append((out.detach(), x.grad))
    (out_a, grad_a), (out_b, grad_b) = results
    assert torch.equal(out_a, out_b) and grad_b is not None and torch.equal(grad_a, grad_b)
    assert torch.equal(grad_a.float(), (1.25 * mask.float()).bfloat16().float().expand(SHAPE))
