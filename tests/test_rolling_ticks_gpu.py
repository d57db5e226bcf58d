"""Device-resident positions and captured ticks of rolling batches (needs an MI355X): `skr_rolling_advance`,
`RollingBatch(device_positions=True)` and `RollingBatch.capture()`.

The yardstick of a request is the request run ALONE, eagerly, through its own wrapper at batch 1 with its own seed (the helpers are
those of test_rolling_gpu.py, copied).  The step kernels are elementwise and so is `net`, so neither who publishes the index (the host
or the advance kernel) nor where the network runs (eagerly or in a replayed graph) can change a bit: every comparison is
`torch.equal`.  The lone runs of a (kind, dtype, shape) are computed once and shared."""

import ctypes
import functools

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.rolling import RollingBatch, advance_reference
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
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
STAGGERED = [(0, 0, 9, 0, 1.0, 11), (0, 3, 4, 1, 0.5, 12), (1, 5, 6, 2, 0.0, 13), (3, 1, 4, 0, 0.5, 14), (5, 3, 6, 1, 1.0, 15), (5, 7, 9, 2, 0.5, 16)]
THREE_CHUNKS = [(0, 2, 6, 0, 1.0, 5), (1, 0, 4, 1, 0.5, 6), (2, 3, 5, 2, 1.0, 7), (5, 0, 4, 1, 1.0, 8)]


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def net(x, t):  # elementwise, out of place, ignores t: a sample's output does not depend on its batch, and NaN stays in its own slot
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


@functools.lru_cache(maxsize=None)
def yardstick(kind, dtype, shape=(4, 32, 32), which="staggered"):
    """(requests, lone results), computed once per case and shared, never written to.  requests: [(tick, slot, steps, variant, eta,
    seed, latents)]; `staggered`: 4, 6 and 9 steps, three schedules / stochasticities, admitted at ticks 0, 1, 3 and 5; slot 3 is
    reused after its first request left"""
    td, dev, g = DTYPES[dtype], torch.device("cuda:0"), torch.Generator().manual_seed(17)
    requests = [(*entry, torch.randn(shape, generator=g).to(td).to(dev)) for entry in (STAGGERED if which == "staggered" else THREE_CHUNKS)]
    refs = [lone(kind, variant, eta, steps, latents, seed) for _, _, steps, variant, eta, seed, latents in requests]
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs)
    return requests, refs


def serve(batch, kind, requests, tick):
    """admits each request at its tick and calls `tick()` (-> finished slots) until all are done:
    ({request number: result}, ticks made, the tick numbers at which a request was admitted)"""
    results, resident, at_tick, admitted_at = {}, {}, 0, []
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, eta, seed, latents) in enumerate(requests):
            if at == at_tick:
                batch.admit(slot, latents, MAKERS[kind](variants()[variant], eta), steps, seed=seed if kind in STOCHASTIC else None)
                resident[slot] = n
                admitted_at.append(at_tick)
        assert batch.active  # (these plans leave no tick empty, so tick numbers are replay numbers)
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        at_tick += 1
        assert at_tick < 64
    torch.cuda.synchronize()
    return results, at_tick, admitted_at


def host_tick(batch):
    return lambda: batch.step(net(batch.latents, batch.timesteps))


def device_tick(batch):
    def tick():
        batch.advance()
        return batch.step(net(batch.latents, batch.timesteps))

    return tick


def make_batch(kind, dtype, dev, shape=(4, 32, 32), capacity=8, **options):
    example = torch.zeros((capacity, *shape), dtype=DTYPES[dtype], device=dev)
    return RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=capacity, **options)


# ---- the advance kernel ---------------------------------------------------------------------------------------------------
GUARD = 64


@pytest.mark.parametrize("max_steps", [1, 128])
@pytest.mark.parametrize("capacity", [1, 255, 256, 257, 300])
def test_advance_kernel_equals_the_reference(capacity, max_steps, dev):
    lib = _hip.load()
    g = torch.Generator().manual_seed(1000 * capacity + max_steps)
    length = torch.randint(0, max_steps + 1, (capacity,), generator=g, dtype=torch.int32)
    position = (torch.rand(capacity, generator=g) * (length + 2).float()).int() - 1  # -1 .. n
    if capacity >= 8:  # the edges by hand: free, full-length, just finished, negative, inconsistent, first and last row of a run
        length[:7] = torch.tensor([0, max_steps, max_steps, max_steps, max_steps + 1, max_steps, max_steps])
        position[:7] = torch.tensor([0, max_steps, max_steps - 1, -3, 0, 0, max_steps - 1])
    else:
        length[0], position[0] = max_steps, 0
    assert (length == 0).any() or capacity == 1
    times = torch.randint(-(2**31), 2**31 - 1, (capacity * max_steps,), generator=g, dtype=torch.int64).to(torch.int32)  # any bits: NaN payloads too
    garbage_i = torch.randint(-(2**31), 2**31 - 1, (capacity + 2 * GUARD,), generator=g, dtype=torch.int64).to(torch.int32)
    garbage_t = torch.randint(-(2**31), 2**31 - 1, (capacity + 2 * GUARD,), generator=g, dtype=torch.int64).to(torch.int32)
    position_dev, length_dev, times_dev = position.to(dev), length.to(dev), times.to(dev).view(torch.float32)
    index_buf, time_buf = garbage_i.to(dev), garbage_t.to(dev).view(torch.float32)
    index_dev, timesteps_dev = index_buf[GUARD : GUARD + capacity], time_buf[GUARD : GUARD + capacity]
    ref_position, ref_times, times_list = position.tolist(), garbage_t[GUARD : GUARD + capacity].tolist(), times.tolist()
    stream = torch.cuda.current_stream(dev).cuda_stream
    moved = 0
    for launch in range(5):
        assert lib.skr_rolling_advance(position_dev.data_ptr(), length_dev.data_ptr(), times_dev.data_ptr(), index_dev.data_ptr(), timesteps_dev.data_ptr(),
                                       capacity, max_steps, stream) == 0  # fmt: skip
        new_position, ref_index, step_times = advance_reference(ref_position, length.tolist(), times_list, max_steps)
        moved += sum(1 for a, b in zip(ref_position, new_position) if a != b)
        ref_position = new_position
        ref_times = [old if new is None else new for old, new in zip(ref_times, step_times)]
        torch.cuda.synchronize()
        assert torch.equal(position_dev.cpu(), torch.tensor(ref_position, dtype=torch.int32)), launch
        assert torch.equal(index_dev.cpu(), torch.tensor(ref_index, dtype=torch.int32)), launch
        assert torch.equal(timesteps_dev.view(torch.int32).cpu(), torch.tensor(ref_times, dtype=torch.int32)), launch
        for buf, was in ((index_buf, garbage_i), (time_buf.view(torch.int32), garbage_t)):
            assert torch.equal(buf[:GUARD].cpu(), was[:GUARD]) and torch.equal(buf[GUARD + capacity :].cpu(), was[GUARD + capacity :]), launch
    assert moved > 0  # (the state was not all idle)
    assert torch.equal(length_dev.cpu(), length) and torch.equal(times_dev.view(torch.int32).cpu(), times)  # inputs untouched


# ---- captured ticks ---------------------------------------------------------------------------------------------------------
def check_against(results, refs, what):
    assert len(results) == len(refs)
    for n, ref in enumerate(refs):
        assert torch.equal(results[n], ref), (*what, n)


CAPTURED = [(kind, "bf16") for kind in ("euler", "dpm2_sde", "adams4", "unipc3", "unipc2_sde", "spc")] + [("dpm2_sde", "fp16"), ("unipc3", "fp16")]


@pytest.mark.parametrize("kind,dtype", CAPTURED)
def test_captured_ticks_equal_the_lone_runs(kind, dtype, dev):
    requests, refs = yardstick(kind, dtype)
    batch = make_batch(kind, dtype, dev, device_positions=True)
    ticks = batch.capture(net)
    P = ticks.phases
    assert P == batch.keep + 2 == len(ticks.graphs) == len(ticks.outputs)
    assert {"euler": 2, "adams4": 5}.get(kind, P) == P
    results, made, admitted_at = serve(batch, kind, requests, ticks.tick)
    check_against(results, refs, (kind, dtype))
    # every graph replayed at least twice, and requests were admitted in front of different phases (all of them where the plan's
    # four admission ticks 0, 1, 3, 5 can reach them: P <= 3; three of them beyond)
    assert made == ticks.ticks > 2 * P and min(ticks.replays) >= 2 and sum(ticks.replays) == made
    assert len({t % P for t in admitted_at}) >= min(P, 3)
    assert not batch.active and all(batch.free(b) for b in range(8))


@pytest.mark.parametrize("kind", ["dpm2_sde", "unipc3"])
def test_captured_ticks_equal_the_host_published_batch(kind, dev):
    requests, _ = yardstick(kind, "bf16")
    eager = make_batch(kind, "bf16", dev)
    assert not eager.device_positions
    expected, _, _ = serve(eager, kind, requests, host_tick(eager))
    batch = make_batch(kind, "bf16", dev, device_positions=True)
    results, _, _ = serve(batch, kind, requests, batch.capture(net).tick)
    check_against(results, [expected[n] for n in range(len(requests))], (kind,))


def test_eager_device_driven_ticks_equal_the_lone_runs(dev):
    requests, refs = yardstick("adams4", "bf16")
    batch = make_batch("adams4", "bf16", dev, device_positions=True)
    results, made, _ = serve(batch, "adams4", requests, device_tick(batch))
    check_against(results, refs, ("adams4", "eager"))
    assert batch.ticks == made


@pytest.mark.parametrize("captured", [False, True])
def test_sample_of_three_chunks(captured, dev):
    "(3, 32, 64): 3 chunks per sample, the dividing form of the chunk -> sample map, in a batch of 5"
    shape = (3, 32, 64)
    requests, refs = yardstick("dpm3", "bf16", shape, "three_chunks")
    batch = make_batch("dpm3", "bf16", dev, shape=shape, capacity=5, device_positions=True)
    results, _, _ = serve(batch, "dpm3", requests, batch.capture(net).tick if captured else device_tick(batch))
    check_against(results, refs, ("dpm3", captured))


def test_idle_slots_keep_their_bytes_and_read_no_row(dev):
    kind, shape = "unipc3", (4, 32, 32)
    batch = make_batch(kind, "bf16", dev, device_positions=True)
    ticks = batch.capture(net)
    rings = batch._x + batch._state
    assert len(batch._state) == ticks.phases
    for t in rings:
        t.fill_(float("nan"))
    before = [t.clone() for t in rings]
    g = torch.Generator().manual_seed(4)
    mine = {2: (12, 0, torch.randn(shape, generator=g).bfloat16().to(dev)), 5: (5, 1, torch.randn(shape, generator=g).bfloat16().to(dev))}
    for slot, (steps, variant, latents) in mine.items():
        batch.admit(slot, latents, MAKERS[kind](variants()[variant]), steps)
    idle = [b for b in range(8) if b not in mine]
    results = {}
    for n in range(12):
        done = ticks.tick()
        index = batch.index_dev.tolist()
        assert all(index[b] == -1 for b in idle), (n, index)
        assert index[2] == 2 * batch.max_steps + n and (index[5] == 5 * batch.max_steps + n if n < 5 else index[5] == -1)
        for slot in done:
            results[slot] = batch.take(slot)
    torch.cuda.synchronize()
    assert sorted(results) == [2, 5] and ticks.ticks == 12
    for t, was in zip(rings, before):
        view = torch.int16 if t.element_size() == 2 else torch.int32
        assert torch.equal(t[idle].view(view), was[idle].view(view))
    for slot, (steps, variant, latents) in mine.items():  # ... and the NaN next door reached nobody
        assert torch.equal(results[slot], lone(kind, variant, 0.0, steps, latents, None)), slot
    with pytest.raises(ValueError, match="no active slot"):
        ticks.tick()
    assert ticks.ticks == 12


def test_refusals_enqueue_nothing(dev):
    kind, shape = "dpm2_sde", (4, 32, 32)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2)).bfloat16().to(dev)
    host = make_batch(kind, "bf16", dev)
    batch = make_batch(kind, "bf16", dev, device_positions=True)
    batch.admit(1, x, MAKERS[kind](variants()[0]), 2, seed=3)
    out = torch.zeros((8, *shape), dtype=torch.bfloat16, device=dev)

    def refused(call, match):
        held = _hip.trace
        _hip.trace = []
        try:
            with pytest.raises(ValueError, match=match):
                call()
            assert _hip.trace == []
        finally:
            _hip.trace = held

    refused(lambda: host.capture(net), "device_positions=True")
    refused(lambda: host.advance(), "device_positions=True")
    refused(lambda: batch.capture(net), "resident request")
    refused(lambda: batch.step(out), "advance")
    tick = device_tick(batch)
    assert tick() == [] and tick() == [1]
    refused(lambda: batch.capture(net), "resident request")  # finished, not taken
    assert torch.equal(batch.take(1), lone(kind, 0, 1.0, 2, x, 3))
    ticks = batch.capture(net)
    refused(lambda: batch.capture(net), "captured already")
    refused(lambda: batch.step(out), "captured")
    refused(lambda: batch.advance(), "captured")
    refused(ticks.tick, "no active slot")
    assert ticks.ticks == 0 and ticks.replays == [0] * ticks.phases
    batch.admit(4, x, MAKERS[kind](variants()[0]), 2, seed=3)  # the batch served eagerly before the capture: same request, same bits
    assert ticks.tick() == [] and ticks.tick() == [4]
    assert torch.equal(batch.take(4), lone(kind, 0, 1.0, 2, x, 3))
    torch.cuda.synchronize()
