"""In-painting in rolling batches (needs an MI355X): `skr_step_launch_masked_rolling` through the C ABI, and
`RollingBatch(inpaint_mask_shape=...)` with `admit(..., inpaint=(mask, original_samples, noise))`.

The yardstick of every test is code that existed before the masked rolling launch: skr_step_launch_masked on one sample's slices with a
plan that holds exactly the operands present in that sample's row, or the request run ALONE, eagerly, through its own wrapper at batch
1 with `set_inpaint` and its own seed.  The kernels are elementwise, Philox is keyed by the sample's seed and the element's position
within the sample, and present operands are summed in slot order, so nothing a sample gets can depend on who shares its launch: every
comparison is exact (`torch.equal`, on the integer view where the C ABI is compared); there is no tolerance to choose.  The helper
vocabulary (bits, make_plan, decoy, junk_row, upload, SHAPES) is that of tests/test_masked_rows_gpu.py."""

import ctypes
import functools
import math

import pytest
import torch
from test_masked_rows_gpu import SHAPES, bits, decoy, junk_row, make_plan, upload

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
OK, ERR_NULL, ERR_UNSUPPORTED = 0, 1, 7
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
COUNTS = (1, 2, 5, 12, 16)
BATCH = 4


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
class Mixed:
    """One launch of 4 samples: 0 inactive (index -1), 1 a full random row, 2 a ramp-up row (every odd operand slot absent, its slice of
    those operands NaN / inf), 3 a row with zeta0 = 0, zeros among coef1 and (from 5 operands on) a present operand whose coef0 is zero.
    With one operand, samples 2 and 3 get full rows.  The table holds NaN rows around the live ones; row_offset is 2."""

    def __init__(self, name, dtype, n, noisy, dev, seed):
        unit, munit, whole, _ = SHAPES[name]
        self.shape, self.dtype, self.n, self.dev = (BATCH, *unit), dtype, n, dev
        self.g = g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(self.shape, generator=g).to(dtype).to(dev) for _ in range(n)]
        for j in range(1, n, 2):
            self.ops[j][2].fill_(float("nan") if j % 4 == 1 else float("inf"))  # what sample 2's row does not have
        mshape = (1 if whole else BATCH, *munit)
        self.whole = whole
        self.mask = torch.rand(mshape, generator=g).to(dtype).to(dev)  # a soft mask: both forms reach every element
        self.mask_numel, self.batch_stride = lazy.mask_layout(mshape, self.shape)
        self.sample_numel, self.numel = math.prod(unit), math.prod(self.shape)
        self.seeds = torch.tensor([11, 22, 33, 44], dtype=torch.int64, device=dev)
        self.arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.ops])
        self.desc = _hip.StepMaskC(self.mask.data_ptr(), _hip.DTYPE_CODE[dtype], 0, self.mask_numel, self.batch_stride)
        self.stream = _hip.current_stream_ptr(dev)
        self.plan = make_plan(n, dtype, self.sample_numel, noisy)
        self.rows = {1: self.row("full", 7 * 256 + 1), 2: self.row("ramp" if n > 1 else "full", 7 * 256 + 2), 3: self.row("known" if n > 1 else "full", 7 * 256 + 3)}
        self.table = upload([junk_row(), junk_row(), self.rows[1], junk_row(), self.rows[2], self.rows[3], junk_row()], dev)
        self.index = torch.tensor([-1, 0, 2, 3], dtype=torch.int32, device=dev)
        self.row_offset = 2

    def pick(self):
        g = self.g
        return float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # +-[0.1, 2]

    def row(self, kind, stream):
        row = _hip.StepRowC()
        for k in range(self.n):
            row.coef0[k], row.coef1[k] = self.pick(), self.pick()
            if kind == "ramp" and k % 2 == 1:
                row.coef0[k], row.coef1[k] = (0.0, -0.0) if k % 4 == 1 else (-0.0, 0.0)  # absent: zeros of either sign
            if kind == "known" and k % 2 == 0:
                row.coef1[k] = 0.0  # present, but not in the known form
            if kind == "known" and k == 3 and self.n >= 5:
                row.coef0[k] = 0.0  # present through coef1 alone: its fma into s is made all the same
        row.zeta0, row.stream0 = (0.0 if kind == "known" else 0.45), stream
        row.chain, row.zeta1, row.stream1 = float("nan"), float("nan"), 99  # not read
        return row

    def rolling(self, plan):
        out = torch.full(self.shape, 3.0, dtype=self.dtype, device=self.dev)
        rc = _hip.load().skr_step_launch_masked_rolling(ctypes.byref(plan), self.arr, out.data_ptr(), ctypes.byref(self.desc), self.seeds.data_ptr(), self.numel,
                                                        self.table.data_ptr(), self.index.data_ptr(), self.row_offset, self.stream)  # fmt: skip
        assert rc == OK, rc
        return out

    def alone(self, b, noisy):
        "skr_step_launch_masked on sample b's slices: exactly the operands present in its row, in order, with the row's values"
        row = self.rows[b]
        present = [k for k in range(self.n) if row.coef0[k] != 0.0 or row.coef1[k] != 0.0]
        plan = make_plan(len(present), self.dtype, self.sample_numel, noisy)
        for j, k in enumerate(present):
            plan.coef0[j], plan.coef1[j] = row.coef0[k], row.coef1[k]
        plan.zeta0, plan.stream0 = row.zeta0, row.stream0
        arr = (ctypes.c_void_p * len(present))(*[self.ops[k][b].data_ptr() for k in present])
        mask = self.mask[0 if self.whole else b]
        desc = _hip.StepMaskC(mask.data_ptr(), _hip.DTYPE_CODE[self.dtype], 0, self.mask_numel, 0)
        out = torch.empty(self.shape[1:], dtype=self.dtype, device=self.dev)
        rc = _hip.load().skr_step_launch_masked(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), self.seeds[b : b + 1].data_ptr(), self.sample_numel, self.stream)
        assert rc == OK, rc
        return out, present


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_launch_equals_the_lone_masked_launches(name, dtype, dev):
    drew = False
    for n in COUNTS:
        for noisy in (False, True):
            p = Mixed(name, DTYPES[dtype], n, noisy, dev, seed=900 + n)
            got = p.rolling(decoy(p.plan))  # (the plan's own scalars are decoys: the rows decide)
            for b in (1, 2, 3):
                want, present = p.alone(b, noisy)
                if n > 1 and b == 2:
                    assert present == list(range(0, n, 2))
                assert torch.isfinite(want.float()).all(), (name, dtype, n, noisy, b)
                assert torch.equal(bits(got[b]), bits(want)), (name, dtype, n, noisy, b, int((bits(got[b]) != bits(want)).sum()))
            assert torch.equal(bits(got[0]), bits(torch.full(p.shape[1:], 3.0, dtype=p.dtype, device=dev)))  # the inactive sample keeps its bytes
            if noisy and not drew:
                quiet, _ = p.alone(1, False)
                assert not torch.equal(got[1], quiet)  # (the draw takes part)
                drew = True
    torch.cuda.synchronize()


def test_error_codes_are_those_of_the_per_sample_masked_entry(dev):
    "argument checks only: every call is refused before anything is launched, with the code skr_step_launch_masked_indexed_per_sample gives"
    p = Mixed("wraps_twice_in_a_chunk", torch.bfloat16, 3, False, dev, seed=1)
    out = torch.full(p.shape, 7.0, dtype=p.dtype, device=dev)
    lib = _hip.load()
    index = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    sn, mn = p.sample_numel, p.mask_numel
    table = upload([p.rows[1], p.rows[3]], dev)

    def call(entry, rows=table.data_ptr(), idx=index.data_ptr(), n=p.numel, mask_ptr=p.mask.data_ptr(), mask_numel=mn, batch_stride=mn, row_offset=0, out_ptr=out.data_ptr(),
             seeds=p.seeds.data_ptr(), no_desc=False, **fields):  # fmt: skip
        plan = make_plan(3, p.dtype, sn, False)
        for key, value in fields.items():
            setattr(plan, key, value)
        d = _hip.StepMaskC(mask_ptr, _hip.BF16, 0, mask_numel, batch_stride)
        return entry(ctypes.byref(plan), p.arr, out_ptr, None if no_desc else ctypes.byref(d), seeds, n, rows, idx, row_offset, p.stream)

    def both(code, **kwargs):
        mine, theirs = call(lib.skr_step_launch_masked_rolling, **kwargs), call(lib.skr_step_launch_masked_indexed_per_sample, **kwargs)
        assert mine == theirs == code, (kwargs, mine, theirs, code)

    both(OK)  # (the calls below differ from this one in one argument each)
    torch.cuda.synchronize()
    assert not (out == 7.0).all()
    out.fill_(7.0)
    both(ERR_NULL, rows=None)
    both(ERR_NULL, idx=None)
    both(ERR_NULL, no_desc=True)
    both(ERR_NULL, mask_ptr=None)
    both(ERR_NULL, out_ptr=None)
    both(ERR_UNSUPPORTED, out1_dtype=_hip.BF16)
    both(ERR_UNSUPPORTED, acc_f64=1)
    both(ERR_UNSUPPORTED, convert_to=1)
    both(ERR_UNSUPPORTED, convert_from=2)
    both(ERR_UNSUPPORTED, row_offset=-1)
    both(ERR_UNSUPPORTED, sample_numel=35 * 2048, n=BATCH * 35 * 2048, mask_numel=35, batch_stride=35)  # mask_numel % 8 != 0 (refused ahead of any access)
    both(ERR_UNSUPPORTED, n=4096, sample_numel=1024)  # whole chunks, but a sample below a chunk
    try:
        assert lib.skr_set_tuning(b"one_trip", 0) == 0
        both(ERR_UNSUPPORTED)  # there is no grid-stride form
    finally:
        lib.skr_set_tuning(b"one_trip", 1)
    both(ERR_NULL, noise_mode=1, seeds=None)  # a launch that may draw needs seeds whatever its rows hold
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- RollingBatch -----------------------------------------------------------------------------------------------------------------------
W = PD.SkrampleWrapperScheduler
MAKERS = {
    "euler": lambda sch, eta=0.0: W(PT.Euler(), sch),
    "dpm2": lambda sch, eta=0.0: W(PT.DPM(order=2), sch),
    "dpm2_sde": lambda sch, eta=1.0: W(PT.DPM(order=2, stochasticity=eta), sch),
    "dpm3": lambda sch, eta=0.0: W(PT.DPM(order=3), sch),
    "adams4": lambda sch, eta=0.0: W(PT.Adams(order=4), sch),
    "unip2": lambda sch, eta=0.0: W(PT.UniP(order=2), sch),
}
STOCHASTIC = ("dpm2_sde",)
# 4, 6 and 9 steps, three schedules / stochasticities, admitted at ticks 0, 1, 3 and 5; slot 3 is reused after its first request left
# (the admission plan of test_rolling_gpu.staggered)
STAGGERED = [(0, 0, 9, 0, 1.0, 11), (0, 3, 4, 1, 0.5, 12), (1, 5, 6, 2, 0.0, 13), (3, 1, 4, 0, 0.5, 14), (5, 3, 6, 1, 1.0, 15), (5, 7, 9, 2, 0.5, 16)]
THREE_CHUNKS = [(0, 2, 6, 0, 1.0, 5), (1, 0, 4, 1, 0.5, 6), (2, 3, 5, 2, 1.0, 7), (5, 0, 4, 1, 1.0, 8)]
UNIT, MASK = (4, 32, 32), (1, 32, 32)


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def net(x, t):  # elementwise, out of place, ignores t: a sample's output does not depend on its batch, and NaN stays in its own slot
    return x * 0.5 + 0.3 * x.abs()


def lone(kind, variant, eta, steps, latents, seed, inpaint):
    "the request alone: its own wrapper, batch 1, its own seed; `inpaint`: (mask, original, noise) of one sample through set_inpaint, or None"
    w = MAKERS[kind](variants()[variant], eta)
    if inpaint is not None:
        w.set_inpaint(*(t.unsqueeze(0) for t in inpaint))
    w.set_timesteps(steps)
    x = latents.unsqueeze(0)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=[seed] if kind in STOCHASTIC else None, return_dict=False)[0]
    return x[0]


@functools.lru_cache(maxsize=None)
def yardstick(kind, dtype, which="staggered", unit=UNIT, mask=MASK, plain=()):
    """(requests, lone results), computed once per case and shared, never written to.  requests: [(tick, slot, steps, variant, eta,
    seed, latents, inpaint)], each with its own soft mask, original and re-noising tensor; `plain`: the request numbers admitted
    with inpaint=None, whose lone runs have no set_inpaint."""
    td, dev, g = DTYPES[dtype], torch.device("cuda:0"), torch.Generator().manual_seed(17)
    requests = []
    for n, entry in enumerate(STAGGERED if which == "staggered" else THREE_CHUNKS):
        latents, original, noise = (torch.randn(unit, generator=g).to(td).to(dev) for _ in range(3))
        soft = torch.rand(mask, generator=g).to(td).to(dev)
        requests.append((*entry, latents, None if n in plain else (soft, original, noise)))
    refs = [lone(kind, variant, eta, steps, latents, seed, inpaint) for _, _, steps, variant, eta, seed, latents, inpaint in requests]
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs)
    return requests, refs


def serve(batch, kind, requests, tick, before_admit=None):
    "admits each request at its tick and calls `tick()` (-> finished slots) until all are done: {request number: result}"
    results, resident, at_tick = {}, {}, 0
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, eta, seed, latents, inpaint) in enumerate(requests):
            if at == at_tick:
                if before_admit is not None:
                    before_admit(batch, slot)
                batch.admit(slot, latents, MAKERS[kind](variants()[variant], eta), steps, seed=seed if kind in STOCHASTIC else None, inpaint=inpaint)
                resident[slot] = n
        assert batch.active  # (these plans leave no tick empty)
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        at_tick += 1
        assert at_tick < 64
    torch.cuda.synchronize()
    return results


def host_tick(batch, model=net):
    return lambda: batch.step(model(batch.latents, batch.timesteps))


def device_tick(batch):
    def tick():
        batch.advance()
        return batch.step(net(batch.latents, batch.timesteps))

    return tick


def make_batch(kind, dtype, dev, unit=UNIT, mask=MASK, capacity=8, **options):
    example = torch.zeros((capacity, *unit), dtype=DTYPES[dtype], device=dev)
    return RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=capacity, inpaint_mask_shape=mask, **options)


def check(results, refs, what):
    for n, ref in enumerate(refs):
        assert torch.equal(results[n], ref), (*what, n)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(MAKERS))
def test_staggered_inpainting_requests_equal_their_lone_runs(kind, dtype, dev):
    requests, refs = yardstick(kind, dtype)
    batch = make_batch(kind, dtype, dev)
    assert ("orig",) in batch.roles and ("znoise",) in batch.roles
    check(serve(batch, kind, requests, host_tick(batch)), refs, (kind, dtype))
    assert not batch.active and all(batch.free(b) for b in range(8))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(MAKERS))
def test_plain_requests_share_a_masked_batch(kind, dtype, dev):
    "half the requests are admitted with inpaint=None: those equal their plain lone runs (no set_inpaint), the others their masked ones"
    requests, refs = yardstick(kind, dtype, plain=(1, 3, 5))
    assert [r[-1] is None for r in requests] == [False, True, False, True, False, True]
    batch = make_batch(kind, dtype, dev)
    check(serve(batch, kind, requests, host_tick(batch)), refs, (kind, dtype))


@pytest.mark.parametrize("kind", ["adams4", "dpm2_sde"])
def test_poisoned_slot_does_not_reach_an_admitted_request(kind, dev):
    "the slot's slices of every ring tensor, `original` and `noise` are NaN / inf before admission: an absent operand must not be read"
    requests, refs = yardstick(kind, "bf16", plain=(1, 3, 5))
    batch = make_batch(kind, "bf16", dev, alias_history=False)

    def poison(batch, slot):
        for n, t in enumerate(batch.ring_tensors() + [batch.latents, batch.original, batch.noise]):
            t[slot].fill_(float("nan") if n % 2 == 0 else float("inf"))

    def model(x, t):  # what a network makes of the leftovers in free slots: NaN there, in the caller's own output tensor too
        out = net(x, t)
        idle = [b for b in range(8) if b not in batch.active]
        if idle:
            out[idle] = float("nan")
        return out

    check(serve(batch, kind, requests, host_tick(batch, model), before_admit=poison), refs, (kind,))


def test_chunk_count_per_sample_not_a_power_of_two(dev):
    "(3, 32, 64): 3 chunks per sample, the dividing form of the chunk -> sample map; the (1, 32, 64) mask wraps once per chunk"
    unit, mask = (3, 32, 64), (1, 32, 64)
    requests, refs = yardstick("dpm2_sde", "bf16", "three_chunks", unit, mask)
    batch = make_batch("dpm2_sde", "bf16", dev, unit, mask, capacity=4)
    check(serve(batch, "dpm2_sde", requests, host_tick(batch)), refs, ("three chunks",))


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams4"])
def test_synchronous_masked_batch_equals_the_per_sample_captured_inpainting_loop(kind, dev):
    shape, steps, seeds = (8, *UNIT), 6, list(range(21, 29))
    g = torch.Generator().manual_seed(31)
    x0, orig, nz = (torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(3))
    mask = torch.rand((8, *MASK), generator=g).bfloat16().to(dev)
    etas = [1.0, 0.5, 1.0]

    def wrapper(k):
        w = MAKERS[kind](variants()[k], etas[k])
        w.set_inpaint(mask, orig, nz)
        return w

    loop = capture_sampling_loop(wrapper(0), net, x0, steps, seeds=seeds, indexed=True, slots=3, per_sample=True)
    for k in (1, 2):
        loop.retarget(wrapper(k), slot=k)
    slot = [2, 0, 1, 1, 0, 2, 0, 1]
    ref = loop(x0, slot=slot)
    batch = make_batch(kind, "bf16", dev)
    requests = [(0, b, steps, k, etas[k], seeds[b], x0[b], (mask[b], orig[b], nz[b])) for b, k in enumerate(slot)]
    results = serve(batch, kind, requests, host_tick(batch))
    for b in range(8):
        assert torch.equal(results[b], ref[b]), (kind, b)


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams4"])
def test_device_positions_and_captured_ticks(kind, dev):
    requests, refs = yardstick(kind, "bf16")
    batch = make_batch(kind, "bf16", dev, device_positions=True)
    check(serve(batch, kind, requests, device_tick(batch)), refs, (kind, "advance + step"))
    batch = make_batch(kind, "bf16", dev, device_positions=True)
    ticks = batch.capture(net)
    check(serve(batch, kind, requests, ticks.tick), refs, (kind, "captured ticks"))


def test_refusals(dev):
    example = torch.zeros((4, *UNIT), dtype=torch.bfloat16, device=dev)
    for sampler in (PT.UniPC(order=2), PT.SPC()):  # their masked step is two launches
        with pytest.raises(_hip.SkrampleHipError, match="not one fused launch"):
            RollingBatch(lambda: W(sampler, variants()[0]), example, capacity=4, inpaint_mask_shape=MASK)
    g = torch.Generator().manual_seed(3)
    x, orig, nz = (torch.randn(UNIT, generator=g).bfloat16().to(dev) for _ in range(3))
    mask = torch.rand(MASK, generator=g).bfloat16().to(dev)
    plain = RollingBatch(lambda: MAKERS["dpm2"](variants()[0]), example, capacity=4)
    with pytest.raises(ValueError, match="inpaint_mask_shape"):
        plain.admit(0, x, MAKERS["dpm2"](variants()[0]), 4, inpaint=(mask, orig, nz))
    batch = make_batch("dpm2", "bf16", dev, capacity=4)
    with pytest.raises(ValueError, match="a mask of shape"):
        batch.admit(0, x, MAKERS["dpm2"](variants()[0]), 4, inpaint=(mask[:, :16], orig, nz))
    with pytest.raises(ValueError, match="original_samples of shape"):
        batch.admit(0, x, MAKERS["dpm2"](variants()[0]), 4, inpaint=(mask, orig.float(), nz))
    assert batch.free(0) and plain.free(0) and bool((batch.mask == 1).all()) and not batch.original.any()
    batch.admit(0, x, MAKERS["dpm2"](variants()[0]), 4, inpaint=(mask > 0.5, orig, nz))  # a bool mask, cast as set_inpaint casts it
    assert torch.equal(batch.mask[0], (mask > 0.5).bfloat16())
    torch.cuda.synchronize()
