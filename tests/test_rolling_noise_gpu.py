"""Offset and Pyramid noise drawn per slot of a rolling batch (needs an MI355X): `skr_noise_offset_rolling`,
`skr_noise_pyramid_rolling` and structured-noise `skrample_amd.rolling.RollingBatch`.

Every comparison is `torch.equal`, and the yardstick is existing code on ONE sample: the whole-batch generator entries at batch 1
(the sample's seed, the streams of its draw number), and the request run alone through its own eager wrapper at batch 1.  Philox is
keyed by the sample's seed and the element's position within the sample, the level geometry and the per-sample statistics are the
sample's own, so what a slot gets cannot depend on its number, its neighbours or which other slots are active."""

import ctypes
import functools

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.pytorch import noise as N
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 5, 7
SUBSTREAMS = 256
CAPACITY, ROWS = 5, 8
DRAWS = [0, None, 3, 7, None]  # slot -> draw number, None: inactive
SEEDS = [0x1234_5678_9ABC_DEF0, 7, (1 << 64) - 3, 99, 1 << 40]
# the pass-1 forms of tests/test_pyramid_routes_gpu.py, at the smallest unit of whole 2048-element chunks that reaches each
PYRAMID_UNITS = {"generic": (4, 32, 32), "strip256": (1, 96, 128), "strip512": (1, 192, 128), "strip1024": (1, 384, 128), "uni": (1, 192, 256)}
OFFSET_UNITS = {"channels": ((4, 32, 32), (0,)), "keeps_innermost": ((4, 32, 32), (0, 2)), "flat": ((2048,), (0,))}


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def seeds_dev(values, dev):
    return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v for v in values], dtype=torch.int64, device=dev)


def index_dev(draws, dev, rows=ROWS):
    return torch.tensor([-1 if d is None else b * rows + d for b, d in enumerate(draws)], dtype=torch.int32, device=dev)


def sentinel(shape, dtype, dev):
    "a tensor of one recognisable bit pattern (not a NaN: compared as integers anyway)"
    fill = {1: 0x5B, 2: 0x4A5B, 4: 0x4A5B4A5B, 8: 0x4A5B4A5B4A5B4A5B}[torch.empty((), dtype=dtype).element_size()]
    as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[torch.empty((), dtype=dtype).element_size()]
    return torch.full(shape, fill, dtype=as_int, device=dev).view(dtype)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class PyramidCase:
    "the workspaces of `batch` samples of one unit, the rolling call and the whole-batch call at batch 1"

    def __init__(self, unit, dtype, dev, batch=CAPACITY, strength=0.3, depth=99):
        self.unit, self.dtype, self.dev, self.batch = unit, dtype, dev, batch
        self.lead, self.h, self.w = unit
        self.numel = self.lead * self.h * self.w
        self.strength, self.depth = strength, depth
        self.lib, self.stream = _hip.load(), _hip.current_stream_ptr(dev)

    def buffers(self, batch):
        return (sentinel((batch, *self.unit), self.dtype, self.dev), sentinel((batch * self.numel,), torch.float32, self.dev),
                sentinel((batch * self.lead * 2,), torch.float64, self.dev), sentinel((batch * 17,), torch.int32, self.dev))  # fmt: skip

    def rolling(self, seeds, index, static, rows=ROWS, stride=SUBSTREAMS, out_dtype=None, index_ptr=True, shape=None):
        out, scratch, partials, levels = self.buffers(self.batch)
        lead, h, w = shape or self.unit
        status = self.lib.skr_noise_pyramid_rolling(out.data_ptr(), _hip.DTYPE_CODE[out_dtype or self.dtype], scratch.data_ptr(), partials.data_ptr(), levels.data_ptr(), seeds.data_ptr(),
                                                    index.data_ptr() if index_ptr else None, rows, stride, 1 if static else 0, self.batch, lead, h, w, 1, self.strength, self.depth, self.stream)  # fmt: skip
        return status, out, scratch, partials, levels

    def alone(self, seed, draw, static):
        out, scratch, partials, levels = self.buffers(1)
        base = draw * SUBSTREAMS
        status = self.lib.skr_noise_pyramid(out.data_ptr(), _hip.DTYPE_CODE[self.dtype], scratch.data_ptr(), partials.data_ptr(), levels.data_ptr(), seeds_dev([seed], self.dev).data_ptr(),
                                            base, 0 if static else base, 1, self.lead, self.h, self.w, 1, self.strength, self.depth, 1, self.stream)  # fmt: skip
        assert status == OK
        return out[0]


class OffsetCase:
    def __init__(self, unit, dims, dtype, dev, batch=CAPACITY, strength=0.6):
        self.unit, self.dtype, self.dev, self.batch, self.strength = unit, dtype, dev, batch, strength
        self.sizes, self.mask = N.Offset._merged(unit, N.OffsetProps(dims=dims))
        self.shape = (ctypes.c_int64 * len(self.sizes))(*self.sizes)
        self.lib, self.stream = _hip.load(), _hip.current_stream_ptr(dev)

    def rolling(self, seeds, index, static, rows=ROWS, stride=SUBSTREAMS, out_dtype=None, index_ptr=True):
        out = sentinel((self.batch, *self.unit), self.dtype, self.dev)
        status = self.lib.skr_noise_offset_rolling(out.data_ptr(), _hip.DTYPE_CODE[out_dtype or self.dtype], seeds.data_ptr(), index.data_ptr() if index_ptr else None, rows, stride,
                                                   1 if static else 0, self.batch, self.shape, len(self.sizes), self.mask, self.strength, self.stream)  # fmt: skip
        return status, out

    def alone(self, seed, draw, static):
        out = sentinel((1, *self.unit), self.dtype, self.dev)
        base = draw * SUBSTREAMS
        status = self.lib.skr_noise_offset(out.data_ptr(), _hip.DTYPE_CODE[self.dtype], seeds_dev([seed], self.dev).data_ptr(), base, 1 if static else base + 1, 1, self.shape,
                                           len(self.sizes), self.mask, self.strength, self.stream)  # fmt: skip
        assert status == OK
        return out[0]


# ---- through the C ABI ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("static", [False, True], ids=["fresh", "static"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("arm", list(PYRAMID_UNITS))
def test_pyramid_slots_equal_the_whole_batch_entry_alone(arm, dtype, static, dev):
    case = PyramidCase(PYRAMID_UNITS[arm], DTYPES[dtype], dev)
    status, out, scratch, partials, levels = case.rolling(seeds_dev(SEEDS, dev), index_dev(DRAWS, dev), static)
    assert status == OK
    untouched = case.buffers(CAPACITY)
    for b, draw in enumerate(DRAWS):
        if draw is not None:
            assert torch.equal(out[b], case.alone(SEEDS[b], draw, static)), (arm, dtype, static, b, draw)
            continue
        # an inactive slot: every buffer keeps its bytes
        for name, got, was, per in (("out", out, untouched[0], 1), ("scratch", scratch, untouched[1], case.numel), ("partials", partials, untouched[2], 2 * case.lead), ("levels", levels, untouched[3], None)):
            if name == "out":
                assert torch.equal(bits(got[b]), bits(was[b])), (arm, name, b)
            elif name == "levels":  # [batch][8][2] sizes, then [batch] counts
                assert torch.equal(got[b * 16 : (b + 1) * 16], was[b * 16 : (b + 1) * 16]) and got[CAPACITY * 16 + b] == was[CAPACITY * 16 + b], (arm, name, b)
            else:
                assert torch.equal(bits(got[b * per : (b + 1) * per]), bits(was[b * per : (b + 1) * per])), (arm, name, b)
    torch.cuda.synchronize()


@pytest.mark.parametrize("static", [False, True], ids=["fresh", "static"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("unit", list(OFFSET_UNITS))
def test_offset_slots_equal_the_whole_batch_entry_alone(unit, dtype, static, dev):
    case = OffsetCase(*OFFSET_UNITS[unit], DTYPES[dtype], dev)
    status, out = case.rolling(seeds_dev(SEEDS, dev), index_dev(DRAWS, dev), static)
    assert status == OK
    untouched = sentinel((CAPACITY, *case.unit), case.dtype, dev)
    for b, draw in enumerate(DRAWS):
        if draw is None:
            assert torch.equal(bits(out[b]), bits(untouched[b])), (unit, b)
        else:
            assert torch.equal(out[b], case.alone(SEEDS[b], draw, static)), (unit, dtype, static, b, draw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("generator", ["pyramid", "offset"])
def test_a_draw_does_not_depend_on_its_slot(generator, dev):
    "the same (seed, draw) in slot 0 and in slot 4, other neighbours active or not"
    seeds = [41, 5, 6, 7, 41]
    case = PyramidCase((4, 32, 32), torch.bfloat16, dev) if generator == "pyramid" else OffsetCase((4, 32, 32), (0,), torch.bfloat16, dev)
    status, out, *_ = case.rolling(seeds_dev(seeds, dev), index_dev([5, None, 2, None, 5], dev), False)
    assert status == OK and torch.equal(out[0], out[4]) and not torch.equal(out[0], out[2])
    status, busy, *_ = case.rolling(seeds_dev(seeds, dev), index_dev([5, 1, 1, 0, 5], dev), False)
    assert status == OK and torch.equal(busy[0], out[0]) and torch.equal(busy[4], out[0])
    assert torch.equal(out[0], case.alone(41, 5, False))
    torch.cuda.synchronize()


def test_refusals_return_their_codes_and_write_nothing(dev):
    seeds, index = seeds_dev(SEEDS, dev), index_dev(DRAWS, dev)
    pyramid, offset = PyramidCase((4, 32, 32), torch.bfloat16, dev), OffsetCase((4, 32, 32), (0,), torch.bfloat16, dev)
    wide = PyramidCase((4, 32, 32), torch.float64, dev), OffsetCase((4, 32, 32), (0,), torch.float64, dev)
    refused = [
        ("no index", ERR_NULL, lambda c: c.rolling(seeds, index, False, index_ptr=False)),
        ("rows_per_slot 0", ERR_SHAPE, lambda c: c.rolling(seeds, index, False, rows=0)),
        ("stream_stride 0", ERR_SHAPE, lambda c: c.rolling(seeds, index, False, stride=0)),
        ("batch * rows_per_slot past INT32_MAX", ERR_SHAPE, lambda c: c.rolling(seeds, index, False, rows=0x7FFFFFFF)),
    ]
    for case in (pyramid, offset):
        for what, code, call in refused:
            status, *buffers = call(case)
            assert status == code, (type(case).__name__, what, status)
            for got in buffers:
                assert torch.equal(bits(got), bits(sentinel(got.shape, got.dtype, dev))), (type(case).__name__, what)
    for case in wide:  # fp64 output: a rolling batch holds no fp64 latents
        status, *buffers = case.rolling(seeds, index, False)
        assert status == ERR_UNSUPPORTED
        for got in buffers:
            assert torch.equal(bits(got), bits(sentinel(got.shape, got.dtype, dev)))
    # a plane the LDS route refuses (the whole-batch entry answers the same, and the Python layer goes to the any-shape kernels)
    odd = PyramidCase((3, 30, 90), torch.bfloat16, dev)
    status, *buffers = odd.rolling(seeds, index, False)
    assert status == ERR_UNSUPPORTED
    for got in buffers:
        assert torch.equal(bits(got), bits(sentinel(got.shape, got.dtype, dev)))
    narrow = OffsetCase((4, 128, 4), (0, 2), torch.bfloat16, dev)  # an innermost axis of 4 that stays its own (kept beside a broadcast one): outside the aligned kernel
    status, out = narrow.rolling(seeds, index, False)
    assert narrow.sizes[-1] == 4 and status == ERR_UNSUPPORTED and torch.equal(bits(out), bits(sentinel(out.shape, out.dtype, dev)))
    # an empty batch: nothing to do, nothing launched
    empty = PyramidCase((4, 32, 32), torch.bfloat16, dev, batch=0)
    assert empty.rolling(seeds, index, False)[0] == OK
    torch.cuda.synchronize()


# ---- through RollingBatch -----------------------------------------------------------------------------------------------------
W = PD.SkrampleWrapperScheduler
SAMPLERS = {
    "dpm2_sde": lambda eta: PT.DPM(order=2, stochasticity=eta),
    "unipc2_sde": lambda eta: PT.UniPC(order=2, stochasticity=eta),
    "euler_sde": lambda eta: PT.Euler(stochasticity=eta),
}
NOISES = {
    "offset": (N.Offset, None),
    "pyramid": (N.Pyramid, None),
    "offset_static": (N.Offset, N.OffsetProps(static=True)),
    "pyramid_static": (N.Pyramid, N.PyramidProps(static=True)),
    "random": (N.Random, None),
}
# 4, 6 and 9 steps, three schedules / stochasticities, admitted at ticks 0, 1, 3 and 5; slot 3 is reused after its first request left
STAGGERED = [(0, 0, 9, 0, 1.0, 11), (0, 3, 4, 1, 0.5, 12), (1, 5, 6, 2, 0.0, 13), (3, 1, 4, 0, 0.5, 14), (5, 3, 6, 1, 1.0, 15), (5, 7, 9, 2, 0.5, 16)]
SHAPE = (4, 32, 32)


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def make(kind, noise, variant=0, eta=1.0, **options):
    noise_type, props = NOISES[noise]
    return W(SAMPLERS[kind](eta), variants()[variant], noise_type=noise_type, noise_props=props, **options)


def net(x, t):  # elementwise, out of place, ignores t: a sample's output does not depend on its batch
    return x * 0.5 + 0.3 * x.abs()


def lone(kind, noise, variant, eta, steps, latents, seed):
    "the request alone: its own wrapper, batch 1, its own seed"
    w = make(kind, noise, variant, eta)
    w.set_timesteps(steps)
    x = latents.unsqueeze(0)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=[seed], return_dict=False)[0]
    return x[0]


@functools.lru_cache(maxsize=None)
def yardstick(kind, noise, dtype):
    "(requests, lone results), computed once per case and shared, never written to.  requests: [(tick, slot, steps, variant, eta, seed, latents)]"
    td, dev, g = DTYPES[dtype], torch.device("cuda:0"), torch.Generator().manual_seed(17)
    requests = [(*entry, torch.randn(SHAPE, generator=g).to(td).to(dev)) for entry in STAGGERED]
    refs = [lone(kind, noise, variant, eta, steps, latents, seed) for _, _, steps, variant, eta, seed, latents in requests]
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs)
    return requests, refs


def serve(batch, kind, noise, requests, tick, before_admit=None):
    "admits each request at its tick and calls `tick()` (-> finished slots) until all are done: {request number: result}"
    results, resident, at_tick = {}, {}, 0
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, eta, seed, latents) in enumerate(requests):
            if at == at_tick:
                if before_admit is not None:
                    before_admit(batch, slot)
                batch.admit(slot, latents, make(kind, noise, variant, eta), steps, seed=seed)
                resident[slot] = n
        assert batch.active  # (the plan leaves no tick empty)
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        at_tick += 1
        assert at_tick < 64
    torch.cuda.synchronize()
    return results


def host_tick(batch):
    return lambda: batch.step(net(batch.latents, batch.timesteps))


def device_tick(batch):
    def tick():
        batch.advance()
        return batch.step(net(batch.latents, batch.timesteps))

    return tick


def make_batch(kind, noise, dtype, dev, capacity=8, **options):
    example = torch.zeros((capacity, *SHAPE), dtype=DTYPES[dtype], device=dev)
    return RollingBatch(lambda: make(kind, noise), example, capacity=capacity, **options)


def check(results, refs, what):
    assert len(results) == len(refs)
    for n, ref in enumerate(refs):
        assert torch.equal(results[n], ref), (*what, n)


CASES = [(k, n, d) for k in SAMPLERS for n in ("offset", "pyramid") for d in ("bf16", "fp16")] + [("dpm2_sde", n, "fp32") for n in ("offset", "pyramid")]


@pytest.mark.parametrize("kind,noise,dtype", CASES)
def test_staggered_requests_equal_their_lone_runs(kind, noise, dtype, dev):
    requests, refs = yardstick(kind, noise, dtype)
    batch = make_batch(kind, noise, dtype, dev)
    assert batch.structured and batch.plan.noise_mode == 0 and ("n",) in batch.roles
    assert (("pn", -1) in batch.roles) == (kind == "unipc2_sde") and len(batch._n) == (len(batch._x) if kind == "unipc2_sde" else 1)
    check(serve(batch, kind, noise, requests, host_tick(batch)), refs, (kind, noise, dtype))
    assert not batch.active and all(batch.free(b) for b in range(8))


@pytest.mark.parametrize("noise", ["offset_static", "pyramid_static"])
def test_static_generators(noise, dev):
    requests, refs = yardstick("dpm2_sde", noise, "bf16")
    batch = make_batch("dpm2_sde", noise, "bf16", dev)
    check(serve(batch, "dpm2_sde", noise, requests, host_tick(batch)), refs, (noise,))
    # (static and fresh generators differ from the second draw on: the case above is not this one again)
    assert not all(torch.equal(a, b) for a, b in zip(refs, yardstick("dpm2_sde", noise.split("_")[0], "bf16")[1]))


@pytest.mark.parametrize("captured", [False, True], ids=["advance_and_step", "captured_ticks"])
@pytest.mark.parametrize("kind,noise", [("dpm2_sde", "pyramid"), ("unipc2_sde", "offset"), ("unipc2_sde", "pyramid"), ("euler_sde", "offset")])
def test_device_positions_and_captured_ticks_equal_the_lone_runs(kind, noise, captured, dev):
    requests, refs = yardstick(kind, noise, "bf16")
    batch = make_batch(kind, noise, "bf16", dev, device_positions=True)
    tick = batch.capture(net).tick if captured else device_tick(batch)
    check(serve(batch, kind, noise, requests, tick), refs, (kind, noise, captured))


@pytest.mark.parametrize("kind,noise", [("unipc2_sde", "pyramid"), ("dpm2_sde", "offset")])
def test_poisoned_noise_of_a_previous_occupant_does_not_reach_a_new_request(kind, noise, dev):
    "every noise tensor's slice of the slot is NaN before each admit (slot 3 is admitted twice): the first row's previous-draw operand is absent, not read"
    requests, refs = yardstick(kind, noise, "bf16")
    batch = make_batch(kind, noise, "bf16", dev)

    def poison(batch, slot):
        for t in batch._n:
            t[slot].fill_(float("nan"))

    check(serve(batch, kind, noise, requests, host_tick(batch), before_admit=poison), refs, (kind, noise))


def test_construction_refusals_name_their_reason(dev):
    example = torch.zeros((4, *SHAPE), dtype=torch.bfloat16, device=dev)
    sde = PT.DPM(order=2, stochasticity=1.0)

    class Custom(N.Offset):
        pass

    for noise_type, match in ((N.Colored, "Colored noise cannot join a rolling batch"), (N.Brownian, "Brownian noise cannot join a rolling batch"), (Custom, "custom generator class")):
        with pytest.raises(_hip.SkrampleHipError, match=match):
            RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=noise_type), example, capacity=4)
    with pytest.raises(ValueError, match="prefetch_noise=True"):
        RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=N.Pyramid, prefetch_noise=True), example, capacity=4)
    with pytest.raises(ValueError, match="inpaint_mask_shape together with Pyramid noise"):
        RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=N.Pyramid), example, capacity=4, inpaint_mask_shape=(1, 32, 32))
    # units the rolling entries do not cover: asked of the route decision, nothing launched
    with pytest.raises(_hip.SkrampleHipError, match="outside the LDS route"):
        RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=N.Pyramid), torch.zeros((2, 1, 512, 512), dtype=torch.bfloat16, device=dev), capacity=2)
    with pytest.raises(_hip.SkrampleHipError, match="no rolling form"):
        RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=N.Pyramid, noise_props=N.PyramidProps(dims=(0, 2))), example, capacity=4)
    with pytest.raises(_hip.SkrampleHipError, match="outside the aligned Offset kernel"):
        RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=N.Offset, noise_props=N.OffsetProps(dims=(0, 2))), torch.zeros((2, 4, 128, 4), dtype=torch.bfloat16, device=dev), capacity=2)
    # a sampler that does not draw: the generator class does not matter, the batch is a plain one
    plain = RollingBatch(lambda: W(PT.DPM(order=2), PS.Scaled(), noise_type=N.Colored), example, capacity=4)
    assert not plain.structured and not plain.draws_noise
    batch = RollingBatch(lambda: W(sde, PS.Scaled(), noise_type=N.Pyramid), example, capacity=4)
    x = torch.zeros(SHAPE, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="noise_props"):
        batch.admit(0, x, W(sde, PS.Scaled(), noise_type=N.Pyramid, noise_props=N.PyramidProps(strength=0.5)), 3, seed=1)
    with pytest.raises(ValueError, match="sampler structure"):
        batch.admit(0, x, W(sde, PS.Scaled(), noise_type=N.Offset), 3, seed=1)
    batch.admit(0, x, W(sde, PS.Scaled(), noise_type=N.Pyramid, noise_props=N.PyramidProps()), 3, seed=1)  # the defaults, spelled out
    torch.cuda.synchronize()


def test_a_random_batch_beside_a_structured_one(dev):
    "both in one process, ticking alternately: no state is shared between the two paths"
    requests, refs = yardstick("dpm2_sde", "random", "bf16")
    other_requests, other_refs = yardstick("dpm2_sde", "pyramid", "bf16")
    plain, structured = make_batch("dpm2_sde", "random", "bf16", dev), make_batch("dpm2_sde", "pyramid", "bf16", dev)
    assert not plain.structured and plain.plan.noise_mode == 1 and structured.plan.noise_mode == 0
    got = {}

    def both():
        if structured.active:
            for slot in structured.step(net(structured.latents, structured.timesteps)):
                got[slot] = structured.take(slot)
        return plain.step(net(plain.latents, plain.timesteps))

    structured.admit(2, other_requests[0][6], make("dpm2_sde", "pyramid", other_requests[0][3], other_requests[0][4]), other_requests[0][2], seed=other_requests[0][5])
    check(serve(plain, "dpm2_sde", "random", requests[:3], both), refs[:3], ("random",))
    assert torch.equal(got[2], other_refs[0])
