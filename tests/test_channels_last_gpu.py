"""Channels-last steps on the device.

C ABI: skr_step_launch_channels_last over channels-last copies of logical tensors gives, viewed logically, the bits skr_step_launch
gives over their contiguous copies -- the draw included, so a seed means the same noise in either memory format.  Every comparison in
this module is bitwise (torch.equal compares logical elements whatever the strides).  The one-trip kernel and the general kernel are
both run on every one-trip case ("one_trip" 0 forces the general one); skr_stat tells which of them a launch took.

Wrapper, sampler and lazy level: steps on channels-last operands run in place -- one launch on the caller's own tensors, a
channels-last result -- and equal the contiguous run; mixed layouts, `lazy.channels_last = False` and masked steps run the path they
ran before."""

import ctypes
import math

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.sampling import lazy
from skrample_amd.sampling import models as PM
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
    return lib.skr_stat(b"channels_last_one_trip"), lib.skr_stat(b"channels_last_general")


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
def make_plan(n, n_a, dtype_a, out0, out1=None, sample_numel=0, coef1=False, chain=0.0, zeta0=0.0, zeta1=0.0, acc_f64=False):
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a = n, n_a
    plan.dtype_a, plan.dtype_b = _hip.DTYPE_CODE[dtype_a], _hip.F64 if acc_f64 else _hip.F32
    plan.out0_dtype = _hip.DTYPE_CODE[out0]
    plan.out1_dtype = _hip.DTYPE_CODE[out1] if out1 is not None else _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k in range(n):
        plan.coef0[k] = (-1.0) ** k * (0.75 + 0.125 * k)
        plan.coef1[k] = (0.3 - 0.21 * k) if coef1 else 0.0
    plan.chain, plan.zeta0, plan.zeta1 = chain, zeta0, zeta1
    plan.stream0, plan.stream1 = 3 * 256, 2**40 + 7 * 256
    plan.noise_mode = 1 if zeta0 != 0.0 or zeta1 != 0.0 else 0
    plan.sample_numel = sample_numel
    return plan


def launch(plan, operands, outs, seeds, layout=None):
    lib = _hip.load()
    numel = operands[0].numel() if operands else outs[0].numel()
    arr = (ctypes.c_void_p * max(len(operands), 1))(*[t.data_ptr() for t in operands])
    ptrs = [o.data_ptr() if o is not None else None for o in outs]
    stream = _hip.current_stream_ptr(outs[0].device)
    if layout is None:
        status = lib.skr_step_launch(ctypes.byref(plan), arr, ptrs[0], ptrs[1], seeds.data_ptr(), numel, stream)
    else:
        status = lib.skr_step_launch_channels_last(ctypes.byref(plan), arr, ptrs[0], ptrs[1], seeds.data_ptr(), ctypes.byref(_hip.StepLayoutC(*layout)), numel, stream)
    assert status == 0, status
    torch.cuda.synchronize()


def operands_of(shape, dtypes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g).to(dt).to(dev) for dt in dtypes]


def empty_cl(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev).contiguous(memory_format=fmt(shape))


def compare(plan, shape, operands, out_dtypes, dev, expect):
    """the contiguous launch against the channels-last launch of the same plan; `expect`: "one_trip", "general" or "forward"
    (which of the new kernels runs, by skr_stat)"""
    seeds = torch.tensor([11 + 2**33 * b for b in range(shape[0])], dtype=torch.int64, device=dev)
    layout = (shape[1], math.prod(shape[2:]))
    want = [torch.full(shape, float("nan"), dtype=dt, device=dev) if dt is not None else None for dt in out_dtypes]
    launch(plan, operands, want, seeds)
    got = [to_cl(torch.full(shape, float("nan"), dtype=dt, device=dev)) if dt is not None else None for dt in out_dtypes]
    before = stats()
    launch(plan, [to_cl(t) for t in operands], got, seeds, layout)
    after = stats()
    assert (after[0] - before[0], after[1] - before[1]) == {"one_trip": (1, 0), "general": (0, 1), "forward": (0, 0)}[expect], (expect, before, after)
    for a, b in zip(got, want):
        if a is not None:
            assert is_cl(a) and not torch.isnan(b.float()).any()
            assert torch.equal(a, b), (shape, float((a.double() - b.double()).abs().max()))
    return want


ONE_TRIP_SHAPES = [(3, 4, 32, 32), (3, 8, 16, 32), (3, 16, 16, 16), (2, 4, 2, 16, 16)]


@pytest.mark.parametrize("shape", ONE_TRIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_trip_cases_equal_the_contiguous_launch_bitwise_on_both_kernels(shape, dtype, dev):
    "(3 samples of two chunks each: the dividing chunk -> sample map and a non-zero `within`)"
    lib = _hip.load()
    sample_numel = math.prod(shape[1:])
    assert sample_numel % 2048 == 0 and (shape[0] != 3 or sample_numel == 4096)
    for n in range(1, 9):  # (with the four shapes and two dtypes: all 48 instantiations of step_kernel_cl1)
        operands = operands_of(shape, [dtype] * n, dev, 100 + n)
        plan = make_plan(n, n, dtype, dtype, sample_numel=sample_numel, zeta0=0.625)
        lib.skr_set_tuning(b"one_trip", 1)
        first = compare(plan, shape, operands, (dtype, None), dev, "one_trip")
        lib.skr_set_tuning(b"one_trip", 0)
        second = compare(plan, shape, operands, (dtype, None), dev, "general")
        lib.skr_set_tuning(b"one_trip", 1)
        assert torch.equal(first[0], second[0])
        # the draw is there: without it the result differs
        quiet = make_plan(n, n, dtype, dtype, sample_numel=sample_numel)
        silent = compare(quiet, shape, operands, (dtype, None), dev, "forward")
        assert not torch.equal(silent[0], first[0])


def test_general_fp32(dev):
    shape = (2, 4, 16, 32)
    operands = operands_of(shape, [torch.float32] * 3, dev, 7)
    compare(make_plan(3, 3, torch.float32, torch.float32, sample_numel=2048, zeta0=-1.25), shape, operands, (torch.float32, None), dev, "general")


def test_general_two_outputs_two_dtype_groups_chain_and_both_draws(dev):
    shape = (2, 4, 32, 32)
    operands = operands_of(shape, [torch.bfloat16] * 4 + [torch.float32], dev, 8)
    plan = make_plan(5, 4, torch.bfloat16, torch.float32, torch.bfloat16, sample_numel=4096, coef1=True, chain=0.8125, zeta0=0.5, zeta1=-0.375)
    compare(plan, shape, operands, (torch.float32, torch.bfloat16), dev, "general")


def test_general_fp64_arithmetic(dev):
    shape = (2, 4, 16, 32)
    operands = operands_of(shape, [torch.bfloat16] * 2 + [torch.float64], dev, 9)
    plan = make_plan(3, 2, torch.bfloat16, torch.float64, torch.bfloat16, sample_numel=2048, coef1=True, chain=-0.25, zeta0=0.5, zeta1=0.75, acc_f64=True)
    compare(plan, shape, operands, (torch.float64, torch.bfloat16), dev, "general")


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (2, 8, 3, 3), (3, 4, 8, 10)], ids=["C=3", "plane%4!=0", "ragged"])
def test_general_odd_channel_counts_planes_and_sizes(shape, dev):
    "C = 3; a plane that is no multiple of 4 (a Philox block then spans two channels); 960 elements, no multiple of 2048"
    sample_numel = math.prod(shape[1:])
    assert sample_numel % 8 == 0
    operands = operands_of(shape, [torch.bfloat16] * 2, dev, 10)
    compare(make_plan(2, 2, torch.bfloat16, torch.bfloat16, sample_numel=sample_numel, zeta0=1.5), shape, operands, (torch.bfloat16, None), dev, "general")


def test_a_launch_without_a_draw_is_the_contiguous_launch_on_the_same_storage(dev):
    shape = (3, 4, 32, 32)
    operands = [to_cl(t) for t in operands_of(shape, [torch.bfloat16] * 3, dev, 12)]
    seeds = torch.zeros(3, dtype=torch.int64, device=dev)
    for plan in (make_plan(3, 3, torch.bfloat16, torch.bfloat16, sample_numel=4096),
                 make_plan(3, 3, torch.bfloat16, torch.float32, torch.bfloat16, sample_numel=4096, coef1=True, chain=0.5)):  # fmt: skip
        dts = (torch.bfloat16, None) if plan.out1_dtype == _hip.NONE else (torch.float32, torch.bfloat16)
        want = [empty_cl(shape, dt, dev) if dt is not None else None for dt in dts]
        got = [empty_cl(shape, dt, dev) if dt is not None else None for dt in dts]
        launch(plan, operands, want, seeds)  # (storage order in, storage order out: the plain entry does not look at strides)
        before = stats()
        launch(plan, operands, got, seeds, (4, 1024))
        assert stats() == before
        for a, b in zip(got, want):
            assert a is None or torch.equal(a, b)


def test_programs_remember_the_layout(dev):
    lib = _hip.load()
    shape, n = (3, 8, 16, 32), 4
    operands = operands_of(shape, [torch.bfloat16] * n, dev, 13)
    plan = make_plan(n, n, torch.bfloat16, torch.bfloat16, sample_numel=4096, zeta0=0.625)
    seeds = torch.tensor([5, 6, 7], dtype=torch.int64, device=dev)
    want = torch.empty(shape, dtype=torch.bfloat16, device=dev)
    plan.stream0 = 9 * 256
    launch(plan, operands, [want, None], seeds)
    plan.stream0 = 0
    handle = ctypes.c_void_p()
    assert lib.skr_program_create_channels_last(ctypes.byref(plan), want.numel(), ctypes.byref(_hip.StepLayoutC(8, 512)), ctypes.byref(handle)) == 0
    cl = [to_cl(t) for t in operands]
    got = empty_cl(shape, torch.bfloat16, dev)
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in cl])
    before = stats()
    assert lib.skr_program_launch(handle.value, arr, got.data_ptr(), None, seeds.data_ptr(), 9 * 256, 0, _hip.current_stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    lib.skr_program_destroy(handle.value)
    assert stats()[0] == before[0] + 1 and torch.equal(got, want)


# ---- the scheduler wrapper -----------------------------------------------------------------------------------------------------------
SHAPE, STEPS, SEEDS = (2, 4, 32, 32), 6, [1234, 2**40 + 5]
WRAPPERS = {
    # (alias_history=True: the history is the caller's own tensors from the first step on, so no snapshot is ever cloned)
    "euler_eta1": lambda: PD.SkrampleWrapperScheduler(PT.Euler(stochasticity=1), PS.Scaled()),
    "dpm2_eta0": lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()), alias_history=True),
    "dpm2_eta1": lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), alias_history=True),
    "adams3": lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled(), alias_history=True),
    "unipc2_eta0": lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=2), PS.Scaled(), alias_history=True),
    "unipc2_eta1": lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=2, stochasticity=1), PS.Linear(), PM.FlowModel(), alias_history=True),
}


def wrapper_inputs(dev, seed=41):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(SHAPE, generator=g).bfloat16().to(dev)
    outs = [torch.randn(SHAPE, generator=g).bfloat16().to(dev) for _ in range(STEPS)]
    return x0, outs


def run(w, x0, outs, traced=False):
    "[(prev_sample, trace entries)] of one loop; traced: every step under a `_hip.trace` list (the general path)"
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


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_wrapper_steps_run_in_place_on_channels_last_latents(name, dev):
    x0, outs = wrapper_inputs(dev)
    x0_cl, outs_cl = to_cl(x0), [to_cl(o) for o in outs]
    want = run(WRAPPERS[name](), x0, outs)
    w = WRAPPERS[name]()
    got = run(w, x0_cl, outs_cl, traced=True)
    known = {x0_cl.data_ptr()} | {o.data_ptr() for o in outs_cl}
    for i, ((a, entries), (b, _)) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and torch.equal(a, b), (name, i)
        assert is_cl(a) and b.is_contiguous(), (name, i)
        assert len(entries) == 1, (name, i, len(entries))  # one launch
        plan, operands, out0, out1 = entries[0][:4]
        for t in operands:  # the caller's tensors, or what an earlier step of this loop wrote: no copy has been made
            assert t.data_ptr() in known and lazy.layout_of(t) == (4, 1024), (name, i)
        for o in (out0, out1):
            if o is not None:
                assert lazy.layout_of(o) == (4, 1024), (name, i)
                known.add(o.data_ptr())
        if name.startswith("unipc") and i > 0:
            assert out1 is not None and out0.dtype == torch.float32 and is_cl(out0), (name, i)  # the fp32 state is channels-last too
    # a second and a third run of the same scheduler: the replayed fast path serves them, and equals a twin that never takes it
    twin = WRAPPERS[name]()
    twin.fast_steps = False
    slow = run(twin, x0_cl, outs_cl)
    hits = w._fast_hits
    for rep in range(2):
        fast = run(w, x0_cl, outs_cl)
        for i, ((a, _), (b, _), (c, _)) in enumerate(zip(fast, slow, want)):
            assert torch.equal(a, b) and torch.equal(a, c) and is_cl(a) and is_cl(b), (name, rep, i)
    assert w._fast_hits > hits and twin._fast_hits == 0, (name, w._fast_hits, hits)


def test_sampler_level_dpm2_sde_with_philox_noise(dev):
    """PT.DPM(order=2, stochasticity=1).sample(...) on channels-last tensors equals the contiguous call.  (Under a compute scale, as the
    wrapper calls it: without one a 16-bit contiguous call replays the reference's rounded ops on the op tape, which takes contiguous
    operands only -- a channels-last call lands on the fused form, as it did before.)"""
    sampler, schedule, model = PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), PM.NoiseModel()
    x0, outs = wrapper_inputs(dev, 43)
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=dev)
    results = {}
    for layout in ("contiguous", "channels_last"):
        conv = to_cl if layout == "channels_last" else (lambda t: t)
        x, previous, traj = conv(x0), [], []
        with lazy.compute_scale(torch.float32):
            for i in range(4):
                noise = lazy.PhiloxNoise(seeds, i * 256, SHAPE, dev)
                rec = sampler.sample(x, conv(outs[i]), Step.from_int(i, 4), model, schedule, noise=noise, previous=previous)
                previous, x = [rec], rec.final
                traj.append(x)
        results[layout] = traj
    for i, (a, b) in enumerate(zip(results["channels_last"], results["contiguous"])):
        assert torch.equal(a, b) and is_cl(a) and b.is_contiguous(), i
    assert not torch.equal(results["contiguous"][0], results["contiguous"][1])


# ---- paths that stay what they were ----------------------------------------------------------------------------------------------------
def test_mixed_layouts_return_the_contiguous_result(dev):
    x0, outs = wrapper_inputs(dev, 44)
    make = WRAPPERS["dpm2_eta1"]
    want = run(make(), x0, outs)
    got = run(make(), x0, [to_cl(o) for o in outs])  # channels-last model outputs, contiguous sample
    for i, ((a, _), (b, _)) in enumerate(zip(got, want)):
        assert torch.equal(a, b) and a.is_contiguous(), i


def test_the_switch_restores_the_copying_path(dev):
    x0, outs = wrapper_inputs(dev, 45)
    make = WRAPPERS["dpm2_eta1"]
    want = run(make(), x0, outs)
    lazy.channels_last = False
    before = stats()
    got = run(make(), to_cl(x0), [to_cl(o) for o in outs])
    assert stats() == before  # no channels-last launch
    for i, ((a, _), (b, _)) in enumerate(zip(got, want)):
        assert torch.equal(a, b) and a.is_contiguous(), i


def test_inpainting_on_channels_last_latents_equals_its_contiguous_run(dev):
    x0, outs = wrapper_inputs(dev, 46)
    g = torch.Generator().manual_seed(47)
    orig, nz = (torch.randn(SHAPE, generator=g).bfloat16().to(dev) for _ in range(2))
    mask = (torch.rand((SHAPE[0], 1, *SHAPE[2:]), generator=g) > 0.5).to(dev)
    results = []
    for conv in ((lambda t: t), to_cl):
        w = WRAPPERS["dpm2_eta1"]()
        w.set_inpaint(mask, conv(orig), conv(nz))
        results.append(run(w, conv(x0), [conv(o) for o in outs]))
    for i, ((a, _), (b, _)) in enumerate(zip(*results)):
        assert torch.equal(a, b), i
