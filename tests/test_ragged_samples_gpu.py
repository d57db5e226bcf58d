"""Ragged samples (needs an MI355X): the table launches on samples that are NOT whole 2048-element chunks -- csrc/skr_step_ragged.hip
behind skr_step_launch_indexed, skr_step_launch_indexed_per_sample and skr_step_launch_rolling -- and what they open in
`RollingBatch` and `capture_sampling_loop`.

Through the C ABI the yardstick is `skr_step_launch` called per sample, on that sample's slices, with the row's values in the plan
and, for a rolling row, exactly its present operands in slot order: a lone sample of such a size is no whole-chunk launch, so the
grid-stride / general kernels of csrc/skr_step.hip take those calls and the code under test is never its own yardstick.  At wrapper
level the yardstick is the request's lone eager `step()` loop.  Every comparison is `torch.equal`; there is no tolerance to choose.

Operands and the output are views of one poisoned allocation with guard bands (tests/arena.py): the poison is NaN in every dtype, so
an element the launch did not write fails the comparison, an inactive slot must still hold it, and no band byte may change.

Sizes (batch 3, so that numel is ragged as well): the smallest at which each liveness boundary occurs --
  2048+8     one live lane vector in the second chunk            2048+256   fp32: all of wave 0's group0, no group1
  2048+264   fp32: two lanes of group1                           2048+1024  two live waves, two dead
  4096-8     one dead lane vector                                2*2048+8   bps = 3: the dividing chunk -> sample form
  64512      (4,144,112): bps = 32, the shift form"""

import ctypes

import pytest
import table_cases as TC
import torch
from arena import Arena, untouched

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.pytorch import noise as PN
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu

BATCH = 3
SIZES = (2048 + 8, 2048 + 256, 2048 + 264, 2048 + 1024, 4096 - 8, 2 * 2048 + 8, 64512)
COUNTS = (1, 4, 5, 12, 13, 16)  # the kernarg-size edges, and the 12-loads-in-flight rule of 16-bit launches from 13 operands on
UNSUPPORTED = _hip.SKR_ERR_UNSUPPORTED
BAND = 64 * 1024


@pytest.fixture(scope="module")
def lib():
    return _hip.load()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---- shared inputs and yardsticks -------------------------------------------------------------------------------------------------
_boxes: dict = {}
_refs: dict = {}
_tables: dict = {}


class Box:
    "16 operands and one output of BATCH samples of `sn` elements, all views of one poisoned arena; the samples' seeds"

    def __init__(self, dtype: str, sn: int, dev):
        self.td, self.sn, self.n = TC.DTYPES[dtype], sn, BATCH * sn
        size = torch.empty(0, dtype=self.td).element_size()
        self.arena = Arena(dev, BAND, 17 * (self.n * size + 2 * BAND + 64) + BAND)
        g = torch.Generator().manual_seed(sn * 3 + size)
        self.ops = []
        for j in range(TC.ROW_TERMS):
            view = self.arena.take(f"in{j}", self.n, self.td)
            view.copy_((torch.randn(self.n, generator=g) * (0.5 + 0.25 * (j % 5))).to(self.td))
            self.ops.append(view)
        self.out = self.arena.take("out", self.n, self.td)
        self.seeds = TC.seeds_tensor(TC.seeds_for(BATCH)).to(dev)

    def poison_out(self) -> None:
        self.out.view(torch.uint8).fill_(0xFF)

    def part(self, t: torch.Tensor, b: int) -> torch.Tensor:
        return t[b * self.sn : (b + 1) * self.sn]


def box_of(dtype: str, sn: int, dev) -> Box:
    if (dtype, sn) not in _boxes:
        _boxes[dtype, sn] = Box(dtype, sn, dev)
    return _boxes[dtype, sn]


def table_of(k: int, noise: str):
    "the rows of tests/table_cases.py for k operands: six dense ones (row 1 skips its draw), then the sparse rows of a rolling table"
    if (k, noise) not in _tables:
        case = TC.Case("k1", k, noise=noise)
        rows, present = TC.build_rows(case, rolling=True)
        _tables[k, noise] = (case, rows, present)
    return _tables[k, noise]


def yardstick(lib, box: Box, dtype: str, k: int, noise: str, r: int, b: int) -> torch.Tensor:
    "sample b alone under row r through skr_step_launch: computed once, shared by every form, never changed"
    key = (dtype, box.sn, k, noise, r, b)
    if key not in _refs:
        case, rows, present = table_of(k, noise)
        plan = TC.make_plan(case, _hip.DTYPE_CODE[box.td], box.sn)
        one = TC.narrow_plan(case, plan, rows[r], present[r])
        ref = torch.full((box.sn,), float("nan"), dtype=box.td, device=box.out.device)
        ptrs = (ctypes.c_void_p * len(present[r]))(*[box.part(box.ops[j], b).data_ptr() for j in present[r]])
        stream = torch.cuda.current_stream(box.out.device).cuda_stream
        assert lib.skr_step_launch(ctypes.byref(one), ptrs, ref.data_ptr(), None, box.seeds[b : b + 1].data_ptr(), box.sn, stream) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(ref.float()).all(), key
        _refs[key] = ref
    return _refs[key]


ENTRIES = {"whole": "skr_step_launch_indexed", "per_sample": "skr_step_launch_indexed_per_sample", "rolling": "skr_step_launch_rolling"}


def launch(lib, form: str, box: Box, k: int, noise: str, picks, off: int) -> None:
    "one table launch of the form on the box's operands into its (poisoned) output; the plan's own scalars are garbage"
    case, rows, _ = table_of(k, noise)
    dev = box.out.device
    plan = TC.make_plan(case, _hip.DTYPE_CODE[box.td], box.sn)
    rows_dev = TC.rows_tensor(rows).to(dev)
    index = torch.tensor(picks, dtype=torch.int32, device=dev)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in box.ops[:k]])
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = getattr(lib, ENTRIES[form])(ctypes.byref(plan), ptrs, box.out.data_ptr(), None, box.seeds.data_ptr() if case.draws else None, box.n,
                                     rows_dev.data_ptr(), index.data_ptr(), off, stream)  # fmt: skip
    assert rc == 0, (form, box.sn, k, noise, picks, off, rc)
    torch.cuda.synchronize()


def check_samples(lib, box: Box, dtype: str, k: int, noise: str, rows_of_samples, where) -> None:
    "rows_of_samples[b]: the table row sample b ran under, or None for an inactive slot, which keeps its poison"
    for b, r in enumerate(rows_of_samples):
        got = box.part(box.out, b)
        if r is None:
            assert untouched(got), (where, b, "an inactive slot was written")
        else:
            assert torch.equal(got, yardstick(lib, box, dtype, k, noise, r, b)), (where, b, r)


# ---- through the C ABI --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(TC.DTYPES))
@pytest.mark.parametrize("sn", SIZES)
def test_indexed_launch_on_ragged_samples(sn, dtype, lib, dev):
    "index 0 and 1, row_offset 0 and 2: rows 0 .. 3 of the table, row 1 with zeta0 = 0 (the whole launch skips its draw)"
    box = box_of(dtype, sn, dev)
    for k in COUNTS:
        for noise in ("on", "off"):
            for idx, off in ((0, 0), (1, 0), (0, 2), (1, 2)):
                box.poison_out()
                launch(lib, "whole", box, k, noise, [idx], off)
                check_samples(lib, box, dtype, k, noise, [idx + off] * BATCH, (sn, dtype, k, noise, idx, off))
    box.arena.check()


@pytest.mark.parametrize("dtype", list(TC.DTYPES))
@pytest.mark.parametrize("sn", SIZES)
def test_per_sample_launch_on_ragged_samples(sn, dtype, lib, dev):
    "a different row for every sample, one of them the row with zeta0 = 0 among noisy rows"
    box = box_of(dtype, sn, dev)
    for k in COUNTS:
        for noise in ("on", "off"):
            for picks, off in (([3, 1, 0], 0), ([1, 4, 2], 1)):
                box.poison_out()
                launch(lib, "per_sample", box, k, noise, picks, off)
                check_samples(lib, box, dtype, k, noise, [p + off for p in picks], (sn, dtype, k, noise, picks, off))
    box.arena.check()


@pytest.mark.parametrize("dtype", list(TC.DTYPES))
@pytest.mark.parametrize("sn", SIZES)
def test_rolling_launch_on_ragged_samples(sn, dtype, lib, dev):
    """an inactive slot between active ones -- so an active ragged slot is directly followed by an inactive one, whose first bytes sit behind
    the neighbour's partly empty last chunk -- and an inactive last slot in front of the guard band; a sparse row whose absent operands'
    buffers hold NaN in that sample's slices"""
    box = box_of(dtype, sn, dev)
    for k in COUNTS:
        for noise in ("on", "off"):
            _, rows, present = table_of(k, noise)
            sparse = list(range(TC.N_DENSE, len(rows)))
            for n, (picks, off) in enumerate((([2, -1, 0], 0), ([0, 3, -2], 1), ([-1, -1, 4], 0))):
                rows_of_samples = [p + off if p >= 0 else None for p in picks]
                if sparse:  # the last active sample runs under a sparse row: its absent operands must not be read
                    b = max(i for i, r in enumerate(rows_of_samples) if r is not None)
                    rows_of_samples[b] = sparse[(n + sn) % len(sparse)]
                    picks = [r - off if r is not None else p for p, r in zip(picks, rows_of_samples)]
                held = []
                for b, r in enumerate(rows_of_samples):
                    for j in (() if r is None else [j for j in range(k) if j not in present[r]]):
                        held.append((j, b, box.part(box.ops[j], b).clone()))
                        box.part(box.ops[j], b).fill_(float("nan"))
                box.poison_out()
                try:
                    launch(lib, "rolling", box, k, noise, picks, off)
                finally:
                    for j, b, was in held:
                        box.part(box.ops[j], b).copy_(was)
                check_samples(lib, box, dtype, k, noise, rows_of_samples, (sn, dtype, k, noise, picks, off))
    box.arena.check()


@pytest.mark.parametrize("form", list(ENTRIES))
@pytest.mark.parametrize("dtype", list(TC.DTYPES))
def test_containment_of_every_ragged_launch(dtype, form, lib, dev):
    "after every single launch: no guard byte changed, every element of an active sample rewritten, an inactive slot still poison"
    for sn in SIZES:
        box = box_of(dtype, sn, dev)
        for k, noise in ((4, "on"), (13, "off")):
            picks, off = {"whole": ([1], 2), "per_sample": ([0, 2, 5], 0), "rolling": ([3, -1, 1], 0)}[form]
            box.poison_out()
            launch(lib, form, box, k, noise, picks, off)
            box.arena.check()
            active = [b for b in range(BATCH) if form != "rolling" or picks[b] >= 0]
            for b in range(BATCH):
                if b in active:
                    left = (box.part(box.out, b).view(torch.uint8) == 0xFF).view(sn, -1).all(dim=1)
                    assert not left.any(), (sn, dtype, form, k, b, "elements never written", int(left.nonzero()[0]))
                else:
                    assert untouched(box.part(box.out, b)), (sn, dtype, form, k, b)
            if form == "rolling":  # the first bytes behind the ragged neighbour's tail
                assert untouched(box.out[sn : sn + 2048])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_refusals_that_stay(dtype, lib, dev):
    "SKR_ERR_UNSUPPORTED with `out` untouched: samples below one chunk or no multiple of 8, and everything but a single-output plan"
    td, code = TC.DTYPES[dtype], _hip.DTYPE_CODE[TC.DTYPES[dtype]]
    sn = 2048 + 264
    arena = Arena(dev, BAND, 8 << 20)
    n_max = BATCH * sn
    ops = [arena.take(f"in{j}", n_max, td) for j in range(4)]
    for t in ops:
        t.fill_(0.5)
    out0, out1 = arena.take("out0", n_max, td), arena.take("out1", n_max, td)
    case, rows, _ = table_of(4, "on")
    rows_dev = TC.rows_tensor(rows).to(dev)
    index = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    seeds = TC.seeds_tensor(TC.seeds_for(BATCH)).to(dev)
    ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ops])
    stream = torch.cuda.current_stream(dev).cuda_stream
    table = (rows_dev.data_ptr(), index.data_ptr(), 0, stream)

    def plan_of(sample: int, noise_mode: int = 1, **fields) -> _hip.StepPlanC:
        plan = TC.make_plan(case, code, sample)
        plan.noise_mode = noise_mode
        for key, value in fields.items():
            setattr(plan, key, value)
        return plan

    for name in ENTRIES.values():
        fn = getattr(lib, name)
        for noise_mode in (1, 0):
            for sample in (1024, 264, 2052):
                plan = plan_of(sample, noise_mode)
                assert fn(ctypes.byref(plan), ptrs, out0.data_ptr(), None, seeds.data_ptr(), BATCH * sample, *table) == UNSUPPORTED, (name, sample, noise_mode)
            two = plan_of(sn, noise_mode, out1_dtype=code)
            assert fn(ctypes.byref(two), ptrs, out0.data_ptr(), out1.data_ptr(), seeds.data_ptr(), BATCH * sn, *table) == UNSUPPORTED, (name, "two outputs")
            conv = plan_of(sn, noise_mode, out1_dtype=code, convert_to=1, convert_from=2)
            assert fn(ctypes.byref(conv), ptrs, out0.data_ptr(), out1.data_ptr(), seeds.data_ptr(), BATCH * sn, *table) == UNSUPPORTED, (name, "conversion")
            wide = plan_of(sn, noise_mode, acc_f64=1)
            assert fn(ctypes.byref(wide), ptrs, out0.data_ptr(), None, seeds.data_ptr(), BATCH * sn, *table) == UNSUPPORTED, (name, "acc_f64")
    # the masked and guided row entries have no ragged form
    mask = _hip.StepMaskC(ops[3].data_ptr(), code, 0, sn, sn)
    guide = _hip.StepGuidanceC(ops[3].data_ptr(), None, 1.5, 0, 0)
    for noise_mode in (1, 0):
        plan = plan_of(sn, noise_mode, n_terms=3, n_group_a=3)
        for name in ("skr_step_launch_masked_indexed", "skr_step_launch_masked_indexed_per_sample", "skr_step_launch_masked_rolling"):
            assert getattr(lib, name)(ctypes.byref(plan), ptrs, out0.data_ptr(), ctypes.byref(mask), seeds.data_ptr(), BATCH * sn, *table) == UNSUPPORTED, name
        for name in ("skr_step_launch_guided_indexed", "skr_step_launch_guided_indexed_per_sample", "skr_step_launch_guided_rolling"):
            assert getattr(lib, name)(ctypes.byref(plan), ptrs, out0.data_ptr(), ctypes.byref(guide), seeds.data_ptr(), BATCH * sn, *table) == UNSUPPORTED, name
    torch.cuda.synchronize()
    assert untouched(out0) and untouched(out1)
    arena.check()


# ---- wrapper level ------------------------------------------------------------------------------------------------------------------
W = PD.SkrampleWrapperScheduler
MAKERS = {
    "euler": lambda sch, eta=0.0: W(PT.Euler(), sch),
    "dpm2_sde": lambda sch, eta=1.0: W(PT.DPM(order=2, stochasticity=eta), sch),
    "adams3": lambda sch, eta=0.0: W(PT.Adams(order=3), sch),
    "unip2": lambda sch, eta=0.0: W(PT.UniP(order=2), sch),
}
STOCHASTIC = ("dpm2_sde",)
UNIT = (4, 24, 24)  # 2304 elements: one chunk and an eighth


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def net(x, t):  # elementwise, ignores t: a sample's output does not depend on its batch
    return x * 0.5 + 0.3 * x.abs()


def lone(kind, variant, eta, steps, latents, seed):
    "the request alone: its own wrapper, batch 1, its own seed, eager step() calls"
    w = MAKERS[kind](variants()[variant], eta)
    w.set_timesteps(steps)
    x = latents.unsqueeze(0)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=[seed] if kind in STOCHASTIC else None, return_dict=False)[0]
    return x[0]


def requests_for(shape, dev, capacity):
    "different ticks, step counts, schedules, stochasticities and seeds; slot 1 is reused after its first request left"
    g = torch.Generator().manual_seed(23)
    plan = [(0, 0, 7, 0, 1.0, 11), (0, 1, 3, 1, 0.5, 12), (1, capacity - 1, 5, 2, 0.0, 13), (4, 1, 4, 0, 0.5, 14), (5, 2, 6, 1, 1.0, 15)]
    return [(*entry, torch.randn(shape, generator=g).bfloat16().to(dev)) for entry in plan]


def serve(batch, kind, requests, ticks=None):
    "admits each request at its tick and steps until all are done -- eagerly, or through captured ticks: {request number: result}"
    results, resident, tick = {}, {}, 0
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, eta, seed, latents) in enumerate(requests):
            if at == tick:
                batch.admit(slot, latents, MAKERS[kind](variants()[variant], eta), steps, seed=seed if kind in STOCHASTIC else None)
                resident[slot] = n
        if batch.active:
            if ticks is not None:
                done = ticks.tick()
            else:
                if batch.device_positions:
                    batch.advance()
                done = batch.step(net(batch.latents, batch.timesteps))
            for slot in done:
                results[resident.pop(slot)] = batch.take(slot)
        tick += 1
        assert tick < 64
    torch.cuda.synchronize()
    return results


@pytest.mark.parametrize("kind", list(MAKERS))
def test_rolling_batch_of_ragged_units_equals_the_lone_runs(kind, dev):
    example = torch.zeros((4, *UNIT), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=4)
    requests = requests_for(UNIT, dev, 4)
    results = serve(batch, kind, requests)
    for n, (_, slot, steps, variant, eta, seed, latents) in enumerate(requests):
        ref = lone(kind, variant, eta, steps, latents, seed)
        assert torch.isfinite(ref.float()).all()
        assert torch.equal(results[n], ref), (kind, n, slot, steps)


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams3"])
def test_rolling_batch_of_ragged_units_with_device_positions_and_captured_ticks(kind, dev):
    example = torch.zeros((4, *UNIT), dtype=torch.bfloat16, device=dev)
    requests = requests_for(UNIT, dev, 4)
    refs = [lone(kind, variant, eta, steps, latents, seed) for (_, _, steps, variant, eta, seed, latents) in requests]
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=4, device_positions=True)
    results = serve(batch, kind, requests)
    for n, ref in enumerate(refs):
        assert torch.equal(results[n], ref), (kind, "advance", n)
    batch = RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=4, device_positions=True)
    results = serve(batch, kind, requests, ticks=batch.capture(net))
    for n, ref in enumerate(refs):
        assert torch.equal(results[n], ref), (kind, "captured ticks", n)


def test_rolling_batch_at_an_sdxl_bucket(dev):
    "(4,144,112): 31.5 chunks a sample, capacity 5"
    unit = (4, 144, 112)
    example = torch.zeros((5, *unit), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(lambda: MAKERS["dpm2_sde"](variants()[0]), example, capacity=5)
    requests = requests_for(unit, dev, 5)
    results = serve(batch, "dpm2_sde", requests)
    for n, (_, slot, steps, variant, eta, seed, latents) in enumerate(requests):
        assert torch.equal(results[n], lone("dpm2_sde", variant, eta, steps, latents, seed)), (n, slot)


def eager_loop(w, x, steps, seeds):
    w.set_timesteps(steps)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=seeds, return_dict=False)[0]
    return x


def test_indexed_capture_serves_ragged_latents(dev):
    "DPM-2 SDE at (3,4,24,24): the captured loop and a re-targeted slot equal their eager loops"
    steps, seeds = 5, [3, 4, 5]
    x0 = torch.randn((3, *UNIT), generator=torch.Generator().manual_seed(9)).bfloat16().to(dev)
    loop = capture_sampling_loop(MAKERS["dpm2_sde"](variants()[0]), net, x0, steps, seeds=seeds, indexed=True, slots=2)
    assert torch.equal(loop(x0), eager_loop(MAKERS["dpm2_sde"](variants()[0]), x0, steps, seeds))
    loop.retarget(MAKERS["dpm2_sde"](variants()[1], 0.5), slot=1)
    assert torch.equal(loop(x0, slot=1), eager_loop(MAKERS["dpm2_sde"](variants()[1], 0.5), x0, steps, seeds))
    assert torch.equal(loop(x0, slot=0), eager_loop(MAKERS["dpm2_sde"](variants()[0]), x0, steps, seeds))
    # a sampler that draws nothing: its launches carry no sample size, and the three samples together are no whole chunks either
    loop = capture_sampling_loop(MAKERS["adams3"](variants()[0]), net, x0, steps, indexed=True, slots=2)
    assert torch.equal(loop(x0), eager_loop(MAKERS["adams3"](variants()[0]), x0, steps, None))


def test_per_sample_capture_serves_ragged_latents(dev):
    "three samples on three different slots: each equals its own eager run"
    steps, seeds, etas = 5, [3, 4, 5], [1.0, 0.5, 1.0]
    x0 = torch.randn((3, *UNIT), generator=torch.Generator().manual_seed(10)).bfloat16().to(dev)
    loop = capture_sampling_loop(MAKERS["dpm2_sde"](variants()[0], etas[0]), net, x0, steps, seeds=seeds, indexed=True, slots=3, per_sample=True)
    for k in (1, 2):
        loop.retarget(MAKERS["dpm2_sde"](variants()[k], etas[k]), slot=k)
    slot = [2, 0, 1]
    got = loop(x0, slot=slot)
    for b, k in enumerate(slot):
        ref = eager_loop(MAKERS["dpm2_sde"](variants()[k], etas[k]), x0[b : b + 1], steps, seeds[b : b + 1])
        assert torch.equal(got[b : b + 1], ref), (b, k)


@pytest.mark.parametrize(
    "options",
    [
        dict(make=lambda: W(PT.UniPC(order=2), PS.Scaled())),
        dict(make=lambda: W(PT.Euler(), PS.Scaled()), guided=True),
        dict(make=lambda: W(PT.Euler(), PS.Scaled()), inpaint_mask_shape=(1, 24, 24)),
        dict(make=lambda: W(PT.DPM(order=2, stochasticity=1), PS.Scaled(), noise_type=PN.Offset)),
    ],
    ids=["unipc", "guided", "inpaint", "offset_noise"],
)
def test_what_a_ragged_rolling_batch_refuses_when_it_is_built(options, dev):
    "each with a message that names ragged samples, and with nothing allocated"
    example = torch.zeros((4, *UNIT), dtype=torch.bfloat16, device=dev)
    options = dict(options)
    make = options.pop("make")
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    with pytest.raises((ValueError, _hip.SkrampleHipError), match="ragged samples"):
        RollingBatch(make, example, capacity=4, **options)
    assert torch.cuda.memory_allocated(dev) == held
