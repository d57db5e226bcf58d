"""Rolling batches (needs an MI355X): `skr_step_launch_rolling` and `skrample_amd.rolling.RollingBatch`.

The yardstick is always the request run ALONE, eagerly, through its own wrapper at batch 1 with its own seed.  The step kernels are
elementwise and Philox is keyed by the sample's seed and the element's position within the sample, so what a request gets cannot
depend on who shares its launches, at which tick it was admitted, or what the slot's previous occupant left behind: every
comparison is `torch.equal`."""

import ctypes

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu

W = PD.SkrampleWrapperScheduler
MAKERS = {
    "euler": lambda sch, eta=0.0: W(PT.Euler(), sch),
    "dpm2_sde": lambda sch, eta=1.0: W(PT.DPM(order=2, stochasticity=eta), sch),
    "dpm3": lambda sch, eta=0.0: W(PT.DPM(order=3), sch),
    "adams4": lambda sch, eta=0.0: W(PT.Adams(order=4), sch),
    "unipc3": lambda sch, eta=0.0: W(PT.UniPC(order=3), sch),
    "unipc2_sde": lambda sch, eta=1.0: W(PT.UniPC(order=2, stochasticity=eta), sch),
    "spc": lambda sch, eta=0.0: W(PT.SPC(), sch),
}
STOCHASTIC = ("dpm2_sde", "unipc2_sde")
TWO_OUTPUTS = ("unipc3", "unipc2_sde", "spc")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def net(x, t):  # elementwise, ignores t: a sample's output does not depend on its batch
    return x * 0.5 + 0.3 * x.abs()


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def lone(kind, variant, eta, steps, latents, seed):
    "the request alone: its own wrapper, batch 1, its own seed"
    w = MAKERS[kind](variants()[variant], eta)
    w.set_timesteps(steps)
    x = latents.unsqueeze(0)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=[seed] if kind in STOCHASTIC else None, return_dict=False)[0]
    return x[0]


def serve(batch, kind, requests, model=net, before_admit=None):
    "requests: [(tick, slot, steps, variant, eta, seed, latents)]; admits each at its tick, steps until all are done: {request number: result}"
    results, resident, tick = {}, {}, 0
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, eta, seed, latents) in enumerate(requests):
            if at == tick:
                if before_admit is not None:
                    before_admit(batch, slot)
                batch.admit(slot, latents, MAKERS[kind](variants()[variant], eta), steps, seed=seed if kind in STOCHASTIC else None)
                resident[slot] = n
        if batch.active:
            for slot in batch.step(model(batch.latents, batch.timesteps)):
                results[resident.pop(slot)] = batch.take(slot)
        tick += 1
        assert tick < 64
    torch.cuda.synchronize()
    return results


def staggered(shape, dev, dtype, g):
    "4, 6 and 9 steps, three schedules / stochasticities, admitted at ticks 0, 1, 3 and 5; slot 3 is reused after its first request left"
    plan = [(0, 0, 9, 0, 1.0, 11), (0, 3, 4, 1, 0.5, 12), (1, 5, 6, 2, 0.0, 13), (3, 1, 4, 0, 0.5, 14), (5, 3, 6, 1, 1.0, 15), (5, 7, 9, 2, 0.5, 16)]
    return [(*entry, torch.randn(shape, generator=g).to(dtype).to(dev)) for entry in plan]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(MAKERS))
def test_staggered_requests_equal_their_lone_runs(kind, dtype, dev):
    shape, td = (4, 32, 32), DTYPES[dtype]
    example = torch.zeros((8, *shape), dtype=td, device=dev)
    make = lambda: MAKERS[kind](variants()[0])  # noqa: E731
    if kind in TWO_OUTPUTS and dtype == "fp32":
        with pytest.raises(_hip.SkrampleHipError, match="request outside kernel coverage"):  # as the whole-batch indexed capture
            RollingBatch(make, example, capacity=8)
        torch.cuda.synchronize()
        return
    batch = RollingBatch(make, example, capacity=8)
    requests = staggered(shape, dev, td, torch.Generator().manual_seed(17))
    results = serve(batch, kind, requests)
    for n, (_, slot, steps, variant, eta, seed, latents) in enumerate(requests):
        ref = lone(kind, variant, eta, steps, latents, seed)
        assert torch.isfinite(ref.float()).all()
        assert torch.equal(results[n], ref), (kind, dtype, n, slot, steps)
    assert not batch.active and all(batch.free(b) for b in range(8))


@pytest.mark.parametrize("kind", ["dpm2_sde", "unipc3", "adams4"])
def test_synchronous_rolling_batch_equals_the_per_sample_captured_loop(kind, dev):
    shape, steps, seeds = (8, 4, 32, 32), 6, list(range(21, 29))
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(31)).bfloat16().to(dev)
    etas = [1.0, 0.5, 1.0]
    loop = capture_sampling_loop(MAKERS[kind](variants()[0], etas[0]), net, x0, steps, seeds=seeds, indexed=True, slots=3, per_sample=True)
    for k in (1, 2):
        loop.retarget(MAKERS[kind](variants()[k], etas[k]), slot=k)
    slot = [2, 0, 1, 1, 0, 2, 0, 1]
    ref = loop(x0, slot=slot)
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), x0, capacity=8)
    results = serve(batch, kind, [(0, b, steps, k, etas[k], seeds[b], x0[b]) for b, k in enumerate(slot)])
    for b in range(8):
        assert torch.equal(results[b], ref[b]), (kind, b)


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams4", "unipc3", "unipc2_sde", "spc"])
def test_poisoned_history_and_state_do_not_reach_an_admitted_request(kind, dev):
    "the slot's slice of every ring tensor is NaN / inf before admission: a zero coefficient is not enough, the operand must not be read"
    shape = (4, 32, 32)
    example = torch.zeros((8, *shape), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=8, alias_history=False)

    def poison(batch, slot):
        for n, t in enumerate(batch.ring_tensors() + [batch.latents]):
            t[slot].fill_(float("nan") if n % 2 == 0 else float("inf"))

    def model(x, t):  # what a network makes of the leftovers in free slots: NaN there, in the caller's own output tensor too
        out = net(x, t)
        idle = [b for b in range(8) if b not in batch.active]
        if idle:
            out[idle] = float("nan")
        return out

    requests = staggered(shape, dev, torch.bfloat16, torch.Generator().manual_seed(5))
    results = serve(batch, kind, requests, model=model, before_admit=poison)
    for n, (_, slot, steps, variant, eta, seed, latents) in enumerate(requests):
        assert torch.equal(results[n], lone(kind, variant, eta, steps, latents, seed)), (kind, n, slot)


@pytest.mark.parametrize("kind", ["dpm2_sde", "unipc3"])
def test_inactive_slots_keep_their_bytes(kind, dev):
    shape = (4, 32, 32)
    example = torch.zeros((8, *shape), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=8)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)
    batch.admit(2, x, MAKERS[kind](variants()[1]), 3, seed=9 if kind in STOCHASTIC else None)
    idle = [0, 1, 3, 4, 5, 6, 7]
    pattern = torch.tensor(0x4A5B, dtype=torch.int16, device=dev).view(torch.bfloat16)
    targets = [batch._x[0]] + ([batch._state[0]] if batch._state else [])  # the tensors the coming launch writes
    for t in targets:
        for b in idle:
            t[b].fill_(0.7109375 if t.dtype != torch.bfloat16 else pattern.item())
    before = [t.clone() for t in targets]
    batch.step(net(batch.latents, batch.timesteps))
    torch.cuda.synchronize()
    assert batch.latents is targets[0]
    for t, was in zip(targets, before):
        assert torch.equal(t[idle].view(torch.int16 if t.element_size() == 2 else torch.int32), was[idle].view(torch.int16 if t.element_size() == 2 else torch.int32))
    assert not torch.equal(targets[0][2], before[0][2])  # the active sample was stepped


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams4"])
def test_chunk_count_per_sample_not_a_power_of_two(kind, dev):
    "(4, 4, 96, 96): 18 chunks per sample, the dividing form of the chunk -> sample map"
    shape = (4, 96, 96)
    example = torch.zeros((4, *shape), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=4)
    g = torch.Generator().manual_seed(3)
    plan = [(0, 2, 6, 0, 1.0, 5), (1, 0, 4, 1, 0.5, 6), (2, 3, 5, 2, 1.0, 7), (5, 0, 4, 1, 1.0, 8)]
    requests = [(*entry, torch.randn(shape, generator=g).bfloat16().to(dev)) for entry in plan]
    results = serve(batch, kind, requests)
    for n, (_, slot, steps, variant, eta, seed, latents) in enumerate(requests):
        assert torch.equal(results[n], lone(kind, variant, eta, steps, latents, seed)), (kind, n, slot)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_rolling_launch_through_the_c_abi(dtype, dev):
    """skr_step_launch_rolling directly: two samples, three rows, one sample inactive at a time; a row with an interior zero coefficient
    whose operand buffer is NaN.  Against one skr_step_launch per active sample on the reduced operand list."""
    lib = _hip.load()
    td, code = (torch.bfloat16, _hip.BF16) if dtype == "bf16" else (torch.float32, _hip.F32)
    batch, sample = 2, 4096
    n = batch * sample
    g = torch.Generator().manual_seed(5)
    ins = [torch.randn(n, generator=g).to(td).to(dev) for _ in range(4)]
    ins[1].fill_(float("nan"))  # the operand that rows 0 and 2 do not have
    ins[3][:sample].fill_(float("inf"))
    seeds = torch.tensor([7, 8], dtype=torch.int64, device=dev)
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.out0_dtype, plan.out1_dtype = 4, 4, code, code, code, -1
    plan.noise_mode, plan.sample_numel = 1, sample
    present = {0: [0, 2, 3], 1: [0, 2], 2: [2]}  # operand 1 (NaN) in none of them; row 1 also lacks the last, row 2 the first
    rows = (_hip.StepRowC * 3)()
    for r, row in enumerate(rows):
        for k in present[r]:
            row.coef0[k] = 0.25 * (k + 1) * (-1) ** r
        row.coef0[1] = -0.0 if r == 1 else 0.0
        row.zeta0, row.stream0 = (0.5, 4 + r) if r != 1 else (0.0, 0)
    rows_dev = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ins])
    stream = torch.cuda.current_stream(dev).cuda_stream
    for picks, off in (([-1, 1], 0), ([1, -1], 0), ([-1, 0], 1), ([2, -1], 0), ([-1, 2], 0), ([1, 2], 0), ([-1, -1], 0), ([-2, 1], 1)):
        index = torch.tensor(picks, dtype=torch.int32, device=dev)
        got = torch.full((n,), 3.0, device=dev, dtype=td)
        assert lib.skr_step_launch_rolling(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, rows_dev.data_ptr(), index.data_ptr(), off, stream) == 0
        ref = torch.full((n,), 3.0, device=dev, dtype=td)  # an inactive sample keeps these bytes
        for b in range(batch):
            if picks[b] < 0:
                continue
            r = picks[b] + off
            if b == 0 and 3 in present[r]:
                continue  # (sample 0's slice of operand 3 is inf: only rows without it are compared there)
            one = _hip.StepPlanC()
            ctypes.memmove(ctypes.byref(one), ctypes.byref(plan), ctypes.sizeof(plan))
            one.n_terms = one.n_group_a = len(present[r])
            for j, k in enumerate(present[r]):
                one.coef0[j] = rows[r].coef0[k]
            one.zeta0, one.stream0 = rows[r].zeta0, rows[r].stream0
            part = (ctypes.c_void_p * len(present[r]))(*[ins[k][b * sample : (b + 1) * sample].data_ptr() for k in present[r]])
            assert lib.skr_step_launch(ctypes.byref(one), part, ref[b * sample : (b + 1) * sample].data_ptr(), None, seeds[b : b + 1].data_ptr(), sample, stream) == 0
        torch.cuda.synchronize()
        for b in range(batch):
            if picks[b] >= 0 and b == 0 and 3 in present[picks[b] + off]:
                continue
            part = slice(b * sample, (b + 1) * sample)
            assert not torch.isnan(got[part]).any() and torch.equal(got[part], ref[part]), (picks, off, b)
    index = torch.zeros(batch, dtype=torch.int32, device=dev)
    got = torch.empty(n, device=dev, dtype=td)
    args = (rows_dev.data_ptr(), index.data_ptr(), 0, stream)
    assert lib.skr_step_launch_rolling(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, rows_dev.data_ptr(), None, 0, stream) == 1
    assert lib.skr_step_launch_rolling(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, None, index.data_ptr(), 0, stream) == 1
    plan.sample_numel = 1024
    assert lib.skr_step_launch_rolling(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, *args) == 7
    plan.sample_numel = 0
    plan.noise_mode = 0
    assert lib.skr_step_launch_rolling(ctypes.byref(plan), ptrs, got.data_ptr(), None, None, n, *args) == 5
    torch.cuda.synchronize()


def test_overwriting_a_held_model_output_raises(dev):
    shape = (4, 32, 32)
    example = torch.zeros((4, *shape), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(lambda: MAKERS["adams4"](variants()[0]), example, capacity=4)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)
    batch.admit(1, x, MAKERS["adams4"](variants()[0]), 6)
    out = net(batch.latents, batch.timesteps)
    batch.step(out)
    out.mul_(2.0)  # the ring still holds it
    with pytest.raises(_hip.SkrampleHipError, match="modified in place"):
        batch.step(net(batch.latents, batch.timesteps))
    batch = RollingBatch(lambda: MAKERS["adams4"](variants()[0]), example, capacity=4)
    batch.admit(1, x, MAKERS["adams4"](variants()[0]), 6)
    static = torch.empty_like(example)
    batch.step(static.copy_(net(batch.latents, batch.timesteps)))
    with pytest.raises(_hip.SkrampleHipError):
        batch.step(static.copy_(net(batch.latents, batch.timesteps)))  # a network with static output memory: use alias_history=False
    snap = RollingBatch(lambda: MAKERS["adams4"](variants()[0]), example, capacity=4, alias_history=False)
    snap.admit(1, x, MAKERS["adams4"](variants()[1]), 4)
    done = []
    while not done:
        done = snap.step(static.copy_(net(snap.latents, snap.timesteps)))
    assert torch.equal(snap.take(1), lone("adams4", 1, 0.0, 4, x, None))
    torch.cuda.synchronize()
