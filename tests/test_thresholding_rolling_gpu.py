"""Dynamic thresholding in rolling batches (needs an MI355X): skr_threshold_scale_rolling and skr_thresholded_step_launch_rolling through the C
ABI, inside an arena, against the direct entries on each slot alone and against float64; `RollingBatch(..., thresholded=True)` against every
request's lone eager `set_thresholding` run; and the refusals."""

import ctypes
import functools
import gc
import math

import numpy as np
import pytest
import torch
from arena import Arena, untouched
from test_thresholding_gpu import plan_for
from test_thresholding_rows_gpu import bits, direct_scale, dtype_id, index_of, row_of, table_of

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.pytorch import noise as generators
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
UNITS = [(4, 16, 32), (4, 32, 32), (4, 32, 48)]  # 1 chunk, 2 chunks (sample_of shifts), 3 chunks (sample_of divides)
CAPACITY = 5
# the table of both ABI tests: slots 0, 2 and 4 active under three rows -- slot 2's the plain clip --, slots 1 and 3 inactive, slot 3's slices NaN
SETTINGS = [(1.25, -0.75, 0.995, 1.5), (1.25, -0.75, 0.995, 1.0), (0.6, -1.5, 0.5, 1e30)]  # (a, b, ratio, maximum) of rows 0, 1, 2
INDEX = [0, -1, 1, -3, 2]  # (every launch passes row_offset = 1: a negative entry is tested before it is added)
ACTIVE = {0: 0, 2: 1, 4: 2}  # slot -> row


def float64_scale(x, o, a, b, ratio, max_value):
    """the header's definition: x0 from three separate fp32 operations, the sorted magnitudes, r = ratio (n - 1), the two ranks interpolated
    in double with the three IEEE operations as written, rounded to fp32 once, min(max(q, 1), maximum)"""
    x0 = np.float32(a) * x.float().cpu().numpy().ravel() + np.float32(b) * o.float().cpu().numpy().ravel()
    assert x0.dtype == np.float32
    mags = np.sort(np.abs(x0)).astype(np.float64)
    r = ratio * (mags.size - 1)
    k = math.floor(r)
    lo, hi = mags[k], mags[min(k + 1, mags.size - 1)]
    return np.minimum(np.maximum(np.float32(lo + (r - k) * (hi - lo)), np.float32(1.0)), np.float32(max_value))


def launched(dtype, n_ops, unit, draws=False, xslot=0, absent=None):
    """both rolling launches over operands [x, o, h...] inside an arena (slot 3's slices NaN): row 2 (slot 4) lacks operand `absent`, whose
    slice of that slot is NaN; row 1 is the plain clip and, where the launch draws, the row whose zeta0 is zero"""
    n, g, arena, slot = math.prod(unit), torch.Generator().manual_seed(10 * n_ops + draws), Arena(DEV), 1
    take = lambda name, dt=dtype: arena.take(name, CAPACITY * n, dt).view(CAPACITY, n)  # noqa: E731
    operands, out, p = [take(f"in{j}") for j in range(n_ops)], take("out"), take("p")
    for t in operands:
        t.copy_((torch.randn(CAPACITY, n, generator=g) * 2).to(dtype))
        t[3].fill_(math.nan)
    scale, workspace = arena.take("scale", CAPACITY, torch.float32), arena.take("workspace", _hip.threshold_workspace(CAPACITY * n, n), torch.uint8)
    coefs = [[f * (0.9 - 0.13 * j) for j in range(n_ops)] for f in (1.0, 0.5, -0.75)]
    if absent is not None:
        coefs[2][absent] = 0.0
        operands[absent][4].fill_(math.nan)
    steps = [(coefs[0], 0.3 if draws else 0.0, 5), (coefs[1], 0.0, 9), (coefs[2], 0.2 if draws else 0.0, 7)]
    tab, index = table_of([row_of(*s, *st) for s, st in zip(SETTINGS, steps)]), index_of(INDEX)
    seeds = torch.tensor([11, 12, 13, 14, 15], dtype=torch.int64, device=DEV) if draws else None
    lib, table, stream = _hip.load(), (tab.data_ptr(), index.data_ptr(), 1), _hip.current_stream_ptr(DEV)
    x, o = operands[xslot], operands[slot]
    status = lib.skr_threshold_scale_rolling(x.data_ptr(), o.data_ptr(), _hip.DTYPE_CODE[dtype], CAPACITY * n, n, *table, scale.data_ptr(), workspace.data_ptr(), stream)
    assert status == 0, status
    plan = plan_for(n_ops, dtype, [0.0] * n_ops, 1.0 if draws else 0.0, n)  # (the plan's scalars are not the rows')
    thr = _hip.StepThresholdC(scale.data_ptr(), p.data_ptr(), 0.0, 0.0, n, slot, xslot, 0)
    status = lib.skr_thresholded_step_launch_rolling(ctypes.byref(plan), _hip._operand_array(operands), out.data_ptr(), ctypes.byref(thr), _hip._ptr(seeds), CAPACITY * n, *table, stream)
    assert status == 0, status
    torch.cuda.synchronize()
    arena.check()
    return n, operands, out, p, scale, workspace, steps, seeds, slot


@pytest.mark.parametrize("unit", UNITS, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_statistic_of_active_slots_and_every_byte_of_the_others(dtype, unit):
    n, (x, o), _, _, scale, workspace, *_ = launched(dtype, 2, unit)
    hist, meta = workspace[: CAPACITY * 8192].view(CAPACITY, 8192), workspace[CAPACITY * 8192 : CAPACITY * 8208].view(CAPACITY, 16)
    candidates = workspace[CAPACITY * 8208 :].view(CAPACITY, 4 * n)
    for b in range(CAPACITY):
        selecting = b in ACTIVE and SETTINGS[ACTIVE[b]][3] > 1.0
        kept = [untouched(t) for t in (scale[b : b + 1], hist[b], meta[b])]
        assert kept == [not selecting] * 3 and (selecting or untouched(candidates[b])), (b, kept)
        if selecting:
            setting = SETTINGS[ACTIVE[b]]
            got = scale[b : b + 1].cpu().numpy().view(np.int32)[0]
            alone = direct_scale(x[b : b + 1].clone(), o[b : b + 1].clone(), *setting).cpu().numpy().view(np.int32)[0]
            ref = float64_scale(x[b], o[b], *setting).view(np.int32)
            print(f"slot {b}: rolling {got:#x} alone {alone:#x} float64 {int(ref):#x}")
            assert got == alone == ref, (b, got, alone, ref)


# (operands, unit, xslot, absent): 2, 3 and 5 operands over the three units, an interior operand absent where there are five; and the wide 16-bit
# form, which keeps 12 loads in flight -- the sample behind them, at 13, and the absent operand at 12
STEP_CASES = [(2, UNITS[0], 0, None), (3, UNITS[1], 0, 2), (5, UNITS[2], 0, 3), (14, UNITS[0], 13, 12)]


@pytest.mark.parametrize("draws", [False, True], ids=["plain", "draw"])
@pytest.mark.parametrize("n_ops,unit,xslot,absent", STEP_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_step_of_active_slots_equals_the_lone_launch_over_the_present_operands(dtype, n_ops, unit, xslot, absent, draws):
    n, operands, out, p, scale, _, steps, seeds, slot = launched(dtype, n_ops, unit, draws, xslot, absent)
    for b in range(CAPACITY):
        if b not in ACTIVE:
            assert untouched(out[b]) and untouched(p[b]) and untouched(scale[b : b + 1]), b
            continue
        (a, w, ratio, max_value), (c, zeta, stream) = SETTINGS[ACTIVE[b]], steps[ACTIVE[b]]
        present = [j for j in range(n_ops) if j in (slot, xslot) or c[j] != 0.0]
        lone, at, xat = [operands[j][b : b + 1].clone() for j in present], present.index(slot), present.index(xslot)
        lone_scale = direct_scale(lone[xat], lone[at], a, w, ratio, max_value) if max_value > 1.0 else None
        lone_plan = plan_for(len(present), dtype, [c[j] for j in present], zeta, n)
        lone_plan.stream0 = stream
        want_out, want_p = torch.empty_like(lone[0]), torch.empty_like(lone[0])
        _hip.launch_step_thresholded(lone_plan, lone, want_out, want_p, lone_scale, a, w, n, at, xat, seeds[b : b + 1].clone() if zeta else None, n, DEV)
        assert torch.isfinite(want_out.float()).all()
        assert torch.equal(bits(out[b]), bits(want_out[0])) and torch.equal(bits(p[b]), bits(want_p[0])), (b, present)


# ---- rolling batches ---------------------------------------------------------------------------------------------------------------------
SAMPLERS = {"euler": PT.Euler, "dpm2": lambda: PT.DPM(order=2), "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1.0), "adams3": lambda: PT.Adams(order=3),
            "unip2": lambda: PT.UniP(order=2)}  # fmt: skip
SCHEDULES = [lambda: PS.Karras(PS.Scaled()), lambda: PS.Scaled(), lambda: PS.Exponential(PS.Scaled())]
# (tick of admission, slot, steps, schedule, seed, (ratio, maximum)): slot 2 is used again once its first request has left, slots 1 and 3 stay free
REQUESTS = [(0, 0, 5, 0, 11, (0.995, 1.5)), (1, 2, 3, 1, 12, (0.9, 3.0)), (2, 4, 4, 2, 13, (0.995, 1.0)), (5, 2, 3, 0, 14, (0.5, 2.0))]


def net(x, t):
    return x * 0.5 + 0.3 * x.abs()


def wrapper_of(name, which=0, setting=(0.995, 1.5), **fields):
    w = PD.SkrampleWrapperScheduler(SAMPLERS[name](), SCHEDULES[which](), **fields)
    w.set_thresholding(*setting)
    return w


@functools.lru_cache(maxsize=None)
def yardstick(name, unit):
    "(latents, lone eager results) of the four requests: computed once per case and shared, never written to"
    g = torch.Generator().manual_seed(17)
    sigma = float(wrapper_of(name).init_noise_sigma)
    latents = [(torch.randn(unit, generator=g) * sigma).bfloat16().to(DEV) for _ in REQUESTS]
    refs = []
    for (_, _, steps, which, seed, setting), x in zip(REQUESTS, latents):
        w = wrapper_of(name, which, setting)
        w.set_timesteps(steps)
        x = x.unsqueeze(0)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=[seed], return_dict=False)[0]
        refs.append(x[0].clone())
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs) and not torch.equal(refs[0], refs[1])
    return latents, refs


@pytest.mark.parametrize("name,unit,captured", [(name, UNITS[i % 3], False) for i, name in enumerate(("euler", "dpm2", "dpm2_sde", "adams3", "unip2"))] + [("dpm2_sde", UNITS[2], True), ("adams3", UNITS[1], True)],
                         ids=lambda v: str(v))  # fmt: skip
def test_every_request_equals_its_lone_eager_run(name, unit, captured):
    latents, refs = yardstick(name, unit)
    example = torch.zeros((CAPACITY, *unit), dtype=torch.bfloat16, device=DEV)
    batch = RollingBatch(lambda: wrapper_of(name), example, capacity=CAPACITY, max_steps=8, thresholded=True, device_positions=captured)
    assert batch.roles[batch.slot] == ("o",) and batch.roles[batch.xslot] == ("x",) and len(batch._p) == (batch.keep + 2 if batch.keep else 0)
    for t in batch.ring_tensors():  # what a previous occupant may have left
        t.fill_(math.nan)
    ticks = batch.capture(net) if captured else None
    tick = ticks.tick if captured else (lambda: batch.step(net(batch.latents, batch.timesteps)))
    results, resident, now = {}, {}, 0
    while len(results) < len(REQUESTS):
        for k, (at, slot, steps, which, seed, setting) in enumerate(REQUESTS):
            if at == now:
                batch.admit(slot, latents[k], wrapper_of(name, which, setting), steps, seed=seed if name == "dpm2_sde" else None)
                resident[slot] = k
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        now += 1
        assert now < 16
    torch.cuda.synchronize()
    for k, ref in enumerate(refs):
        assert torch.equal(bits(results[k]), bits(ref)), (name, unit, k, int((bits(results[k]) != bits(ref)).sum()))
    assert batch._outputs == [] and batch._stamps == []  # nothing of the caller is held
    assert ticks is None or (ticks.ticks > ticks.phases and min(ticks.replays) >= 1)


SAMPLERS.update(unipc2=lambda: PT.UniPC(order=2), spc=PT.SPC)  # (refused)
REFUSED = {
    "UniPC": (lambda: wrapper_of("unipc2"), {}, "UniPC is two launches"),
    "SPC": (lambda: wrapper_of("spc"), {}, "SPC is two launches"),
    "guided": (lambda: wrapper_of("euler"), dict(guided=True), "thresholded together with guided"),
    "inpaint": (lambda: wrapper_of("euler"), dict(inpaint_mask_shape=(1, 16, 32)), "thresholded together with inpaint_mask_shape"),
    "offset": (lambda: wrapper_of("dpm2_sde", noise_type=generators.Offset), {}, "thresholded together with Offset noise"),
    "pyramid": (lambda: wrapper_of("dpm2_sde", noise_type=generators.Pyramid), {}, "thresholded together with Pyramid noise"),
    "compute_scale": (lambda: wrapper_of("euler", compute_scale=None), {}, "compute_scale=None"),
    "fp64": (lambda: wrapper_of("euler"), dict(dtype=torch.float64), "fp64"),
    "ragged": (lambda: wrapper_of("euler"), dict(unit=(4, 18, 32)), "thresholded together with ragged samples"),
    "runge_kutta": (lambda: PD.RKUltraWrapperScheduler(PS.Karras(PS.Scaled())), {}, "Runge-Kutta"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_when_the_batch_is_built_before_anything_is_allocated(case):
    make, options, says = REFUSED[case]
    options = dict(options)
    example = torch.zeros((2, *options.pop("unit", UNITS[0])), dtype=options.pop("dtype", torch.bfloat16), device=DEV)
    gc.collect()  # (what earlier cases left in reference cycles goes now, not inside the measured window)
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises((_hip.SkrampleHipError, ValueError), match=says):
        RollingBatch(make, example, capacity=2, thresholded=True, **options)
    assert torch.cuda.memory_allocated(DEV) == before
