"""Per-sample schedules (needs an MI355X): `skr_step_launch_indexed_per_sample` and `capture_sampling_loop(..., per_sample=True)`.

The bar is bitwise equality.  The step kernels are elementwise and Philox is keyed by the sample's seed and the element's index
within the sample, so what a sample gets cannot depend on the rows its batch neighbours read: sample b of a replay with
`slot=[...]` must equal sample b of the whole-batch replay `slot=slot[b]`, and of the eager wrapper run of that schedule."""

import ctypes

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import CapturedLoops, capture_sampling_loop
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu

MAKERS = {
    "dpm2_sde": lambda sch, eta=1.0: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=eta), sch),
    "unipc3_sde": lambda sch, eta=1.0: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=eta), sch),
    "adams4": lambda sch, eta=0.0: PD.SkrampleWrapperScheduler(PT.Adams(order=4), sch),
    "rk4_sde": lambda sch, eta=1.0: PD.RKUltraWrapperScheduler(sch, sampler_order=4, stochasticity=eta),
    "adams7": lambda sch, eta=0.0: PD.SkrampleWrapperScheduler(PT.Adams(order=7), sch),
    "unipc5_sde": lambda sch, eta=1.0: PD.SkrampleWrapperScheduler(PT.UniPC(order=5, stochasticity=eta), sch),
}
STOCHASTIC = ("dpm2_sde", "unipc3_sde", "rk4_sde", "unipc5_sde")  # kinds whose slots may differ in stochasticity
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Karras(PS.Scaled(), rho=3.0), PS.Exponential(PS.Scaled())]


def steps_of(kind: str) -> int:
    return 10 if kind in ("adams7", "unipc5_sde") else 6


def net(x, t):  # (ignores t, as the network of test_step_gpu.py::test_indexed_graph_serves_other_schedules)
    return x * 0.5 + 0.3 * x.abs()


def net_t(x, t):  # follows t: a 0-d element of the timesteps (whole-batch loops) or one entry per sample
    return (x * (1 + 1e-3 * t.view(-1, 1, 1, 1))).to(x.dtype)


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def schedules_of(kind: str):
    "[(scheduler, stochasticity)] of every slot: the four schedule variants, and for stochastic samplers one more stochasticity"
    mk = MAKERS[kind]
    made = [(lambda sch=sch: mk(sch)) for sch in variants()]
    if kind in STOCHASTIC:
        made.append(lambda: mk(variants()[1], 0.5))
    return made


def loaded_loop(kind, model, x0, seeds, **options):
    "a per-sample loop with every slot loaded"
    made = schedules_of(kind)
    loop = capture_sampling_loop(made[0](), model, x0, steps_of(kind), seeds=seeds, indexed=True, slots=len(made), per_sample=True, **options)
    for slot in range(1, len(made)):
        loop.retarget(made[slot](), slot=slot)
    return loop, made


def slot_vector(slots: int, batch: int) -> list[int]:
    "every slot at least once, not sorted"
    base = [3, 0, 4, 1, 2, 4, 0, 2] if slots == 5 else [3, 0, 2, 1, 2, 1, 0, 3]
    vec = [base[b % len(base)] for b in range(batch)]
    assert batch < slots or set(vec) == set(range(slots))
    assert vec != sorted(vec)
    return vec


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(MAKERS))
def test_per_sample_slots_agree_bitwise(kind, dtype, dev):
    "every sample of a per-sample replay == that sample of the whole-batch replay of its slot == that sample of the eager run"
    shape, steps = (8, 4, 32, 32), steps_of(kind)  # 4096 elements per sample: two chunks
    seeds = list(range(21, 29))
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(shape, generator=g).to(DTYPES[dtype]).to(dev)

    def eager(w, x, use=seeds):
        w.set_timesteps(steps)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=use, return_dict=False)[0]
        return x

    if kind.startswith("unipc") and dtype == "fp32":
        # The per-sample entry covers what skr_step_launch_indexed covers, and the two-output table kernels of UniPC take 16-bit
        # operands: fp32 latents are refused by the whole-batch indexed capture, and in the same way by the per-sample one.
        for options in ({}, {"per_sample": True}):
            with pytest.raises(_hip.SkrampleHipError, match="request outside kernel coverage"):
                capture_sampling_loop(MAKERS[kind](variants()[0]), net, x0, steps, seeds=seeds, indexed=True, **options)
        torch.cuda.synchronize()
        return
    loop, made = loaded_loop(kind, net, x0, seeds)
    assert loop.per_sample and loop.slots == len(made)
    slot = slot_vector(len(made), shape[0])
    out = loop(x0, slot=slot)
    assert torch.isfinite(out.float()).all()
    uniform = {k: loop(x0, slot=k) for k in set(slot)}
    eagers = {k: eager(made[k](), x0) for k in set(slot)}
    for b, k in enumerate(slot):
        assert torch.equal(out[b], uniform[k][b]), (kind, dtype, b, k, "whole-batch replay")
        assert torch.equal(out[b], eagers[k][b]), (kind, dtype, b, k, "eager")
    assert not torch.equal(uniform[0], uniform[1])
    # a vector of one value is the int form (and the loop returns to per-sample slots afterwards)
    assert torch.equal(loop(x0, slot=[2] * shape[0]), uniform[2])
    assert torch.equal(loop(x0, slot=torch.tensor(slot)), out)
    # new seeds and a second latent tensor
    seeds2 = list(range(101, 109)) if kind in STOCHASTIC else seeds  # (a loop that draws no noise takes no seeds)
    x1 = torch.randn(shape, generator=g).to(DTYPES[dtype]).to(dev)
    out2 = loop(x1, seeds=seeds2 if kind in STOCHASTIC else None, slot=slot)
    for k in set(slot):
        ref = eager(made[k](), x1, seeds2)
        for b in (b for b, kb in enumerate(slot) if kb == k):
            assert torch.equal(out2[b], ref[b]), (kind, dtype, b, k, "new seeds and latents")
    if kind in STOCHASTIC:
        assert not torch.equal(out2, loop(x1, seeds=seeds, slot=slot))


@pytest.mark.parametrize("kind", ["dpm2_sde", "unipc3_sde", "rk4_sde"])
def test_network_follows_each_samples_timesteps(kind, dev):
    "device_timesteps on a per-sample loop: the network gets a [batch] t, each entry the timestep of that sample's own schedule"
    shape, steps = (8, 4, 32, 32), steps_of(kind)
    seeds = list(range(41, 49))
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(7)).bfloat16().to(dev)
    seen = []

    def spy(x, t):
        seen.append(tuple(t.shape))
        return net_t(x, t)

    loop, made = loaded_loop(kind, spy, x0, seeds)
    assert set(seen) == {(shape[0],), (1,)}, set(seen)  # the capture hands the network [batch], the re-targeting dry runs [1]
    assert loop.sample_times.shape == (loop.static_times.numel(), shape[0])  # one row per network call (Runge-Kutta: per stage)
    # the whole-batch loops of the same slots: their network reads 0-d elements of the scheduler's timesteps
    uniform_loop = capture_sampling_loop(made[0](), net_t, x0, steps, seeds=seeds, indexed=True, slots=len(made))
    for k in range(1, len(made)):
        uniform_loop.retarget(made[k](), slot=k)
    slot = slot_vector(len(made), shape[0])
    out = loop(x0, slot=slot)
    refs = {k: uniform_loop(x0, slot=k) for k in set(slot)}
    for b, k in enumerate(slot):
        assert torch.equal(out[b], refs[k][b]), (kind, b, k)
    assert not torch.equal(refs[0], refs[1])
    # re-targeting a slot some samples follow rewrites their columns; the others keep theirs
    loop.retarget(made[3](), slot=0)
    out3 = loop(x0, slot=slot)
    for b, k in enumerate(slot):
        assert torch.equal(out3[b], refs[3 if k == 0 else k][b]), (kind, b, k)
    # the int form on a per-sample loop
    assert torch.equal(loop(x0, slot=1), refs[1])


@pytest.mark.parametrize("noise", [True, False])
def test_chunk_count_per_sample_not_a_power_of_two(noise, dev):
    "(4, 4, 96, 96): 18 chunks per sample, the dividing form of the chunk -> sample map"
    kind = "dpm2_sde" if noise else "adams4"
    shape, steps, seeds = (4, 4, 96, 96), steps_of(kind), [5, 6, 7, 8]
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(3)).bfloat16().to(dev)
    loop, made = loaded_loop(kind, net, x0, seeds)
    slot = [2, 0, 3, 1]
    out = loop(x0, slot=slot)
    for b, k in enumerate(slot):
        assert torch.equal(out[b], loop(x0, slot=k)[b]), (b, k)
        w = made[k]()
        w.set_timesteps(steps)
        x = x0
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=seeds, return_dict=False)[0]
        assert torch.equal(out[b], x[b]), (b, k, "eager")


def test_samples_smaller_than_a_chunk_are_refused(dev):
    "(4, 4, 16, 16): 1024 elements per sample -- a workgroup would span two samples"
    x0 = torch.randn(4, 4, 16, 16, generator=torch.Generator().manual_seed(3)).bfloat16().to(dev)
    for kind in ("dpm2_sde", "adams4"):
        with pytest.raises(_hip.SkrampleHipError, match="request outside kernel coverage"):
            capture_sampling_loop(MAKERS[kind](variants()[0]), net, x0, 6, seeds=[1, 2, 3, 4], indexed=True, per_sample=True)
    torch.cuda.synchronize()


def test_captured_loops_pass_per_sample_through(dev):
    shape, seeds = (8, 4, 32, 32), list(range(8))
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(9)).bfloat16().to(dev)
    loops = CapturedLoops(lambda: MAKERS["dpm2_sde"](variants()[0]), net, x0, seeds=seeds, indexed=True, slots=2, per_sample=True)
    loops.loop(6).retarget(MAKERS["dpm2_sde"](variants()[1]), slot=1)
    slot = [1, 0, 0, 1, 1, 0, 1, 0]
    out = loops(x0, 6, slot=slot)
    a, b = loops(x0, 6, slot=0), loops(x0, 6, slot=1)
    for i, k in enumerate(slot):
        assert torch.equal(out[i], (a, b)[k][i])
    with pytest.raises(ValueError, match="never been loaded"):
        loops(x0, 7, slot=slot)  # a new length: its slot 1 holds nothing yet -- refused on the host, nothing enqueued


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_per_sample_launch_through_the_c_abi(dtype, dev):
    """skr_step_launch_indexed_per_sample directly, against one skr_step_launch per sample: two rows, two samples, one row with
    zeta == 0 beside one with zeta != 0 (that sample skips its draw while its neighbour draws)"""
    lib = _hip.load()
    td, code = (torch.bfloat16, _hip.BF16) if dtype == "bf16" else (torch.float32, _hip.F32)
    batch, sample = 2, 4096
    n = batch * sample
    g = torch.Generator().manual_seed(5)
    ins = [torch.randn(n, generator=g).to(td).to(dev) for _ in range(3)]
    seeds = torch.tensor([7, 8], dtype=torch.int64, device=dev)
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.out0_dtype, plan.out1_dtype = 3, 3, code, code, code, -1
    plan.noise_mode, plan.sample_numel = 1, sample
    rows = (_hip.StepRowC * 3)()
    for r, row in enumerate(rows):
        for k in range(3):
            row.coef0[k] = 0.25 * (k + 1) * (-1) ** r
        row.zeta0, row.stream0 = (0.5, 4 + r) if r != 1 else (0.0, 0)
    rows_dev = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ins])
    stream = torch.cuda.current_stream(dev).cuda_stream
    for picks, off in (([0, 1], 0), ([1, 0], 0), ([1, 1], 0), ([0, 0], 0), ([0, 1], 1), ([1, 0], 1)):
        index = torch.tensor(picks, dtype=torch.int32, device=dev)
        got = torch.full((n,), float("nan"), device=dev, dtype=td)
        assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, rows_dev.data_ptr(), index.data_ptr(), off, stream) == 0
        ref = torch.full((n,), float("nan"), device=dev, dtype=td)
        for b in range(batch):
            row = rows[picks[b] + off]
            one = _hip.StepPlanC()
            ctypes.memmove(ctypes.byref(one), ctypes.byref(plan), ctypes.sizeof(plan))
            for k in range(3):
                one.coef0[k] = row.coef0[k]
            one.zeta0, one.stream0 = row.zeta0, row.stream0
            part = (ctypes.c_void_p * 3)(*[t[b * sample : (b + 1) * sample].data_ptr() for t in ins])
            assert lib.skr_step_launch(ctypes.byref(one), part, ref[b * sample : (b + 1) * sample].data_ptr(), None, seeds[b : b + 1].data_ptr(), sample, stream) == 0
        torch.cuda.synchronize()
        assert not torch.isnan(got).any() and torch.equal(got, ref), (picks, off)
    got = torch.empty(n, device=dev, dtype=td)
    index = torch.zeros(batch, dtype=torch.int32, device=dev)
    args = (rows_dev.data_ptr(), index.data_ptr(), 0, stream)
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, rows_dev.data_ptr(), None, 0, stream) == 1  # SKR_ERR_NULL
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, None, index.data_ptr(), 0, stream) == 1
    plan.sample_numel = 1024  # half a chunk: a workgroup would span two samples
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, *args) == 7  # SKR_ERR_UNSUPPORTED
    plan.noise_mode = 0  # ... with or without noise
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, None, n, *args) == 7
    plan.sample_numel = 0  # no sample size, no batch
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, None, n, *args) == 5  # SKR_ERR_SHAPE
    plan.sample_numel = sample
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, got.data_ptr(), None, None, n, *args) == 0  # no noise: no seeds needed
    torch.cuda.synchronize()
