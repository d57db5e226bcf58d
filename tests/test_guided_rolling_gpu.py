"""Guided steps in rolling batches (needs an MI355X): skr_step_launch_guided_rolling through the C ABI, and guided
`skrample_amd.rolling.RollingBatch`es -- per-request scales and guidance schedules, one launch a tick.

The yardstick of every test is code that existed before the entry: skr_step_launch_guided on one sample with the narrowed plan, the
eager `step_guided` run of a lone wrapper, torch's three lines in front of a plain RollingBatch, or
skr_step_launch_guided_indexed_per_sample for the status codes.  Every comparison is therefore bitwise; there is no tolerance to choose."""

import ctypes
import functools

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, rolling
from skrample_amd.pytorch import noise as generators
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- 1. the entry through the C ABI ------------------------------------------------------------------------------------------------
SAMPLES = 5  # 0: inactive, 1: every operand, 2 and 3: two subsets absent (their bytes NaN), 4: zeta0 == 0
COUNTS = (1, 2, 3, 4, 5, 8, 9, 16)  # every guided_kmax bucket and its edges
SCALES = [NAN, 7.3, -2.6, 1.0, 3.3]  # per sample; neither 7.3 nor 3.3 is an fp32 value, one scale is negative


def make_plan(n, dtype, sample_numel, noisy):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = _hip.DTYPE_CODE[dtype]
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel = sample_numel
    plan.noise_mode = 1 if noisy else 0
    return plan


def decoy(plan):
    "the plan a row launch is handed: other, non-zero scalars, which it must ignore"
    p = _hip.StepPlanC.from_buffer_copy(plan)
    for k in range(p.n_terms):
        p.coef0[k], p.coef1[k] = 9.0 + k, -7.0 - k
    p.zeta0, p.stream0 = 5.0, 77
    return p


def junk_row():
    "a row no launch of these tests may read: every double a NaN"
    row = _hip.StepRowC()
    for k in range(_hip.ROW_TERMS):
        row.coef0[k] = row.coef1[k] = NAN
    row.zeta0 = row.chain = row.zeta1 = NAN
    for k in range(4):
        row.convert_k[k] = NAN
    return row


def upload(rows, dev):
    table = torch.zeros(len(rows) * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
    _hip.upload_rows(table, 0, rows)
    return table


def absent_sets(n, slot):
    "the operands sample 2 and sample 3 do not have: two different subsets of the operands other than `slot` (empty when there is no other)"
    others = [k for k in range(n) if k != slot]
    return {1: [], 2: others[0::2], 3: others[1::2] if len(others) > 1 else others, 4: []}


class Problem:
    "the tensors of one sample size and dtype (16 operands: a launch of n takes the first n), shared by every case of a test and never written"

    def __init__(self, sample_numel, dtype, dev, seed):
        self.shape, self.dtype, self.dev, self.sn = (SAMPLES, sample_numel), dtype, dev, sample_numel
        self.g = g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(self.shape, generator=g).to(dtype).to(dev) for _ in range(_hip.ROW_TERMS)]
        self.cond = torch.randn(self.shape, generator=g).to(dtype).to(dev)
        self.seeds = torch.tensor([11, 22, 33, 44, 55], dtype=torch.int64, device=dev)
        self.sentinel = (torch.arange(SAMPLES * sample_numel, device=dev) % 251).reshape(self.shape).to(dtype)
        self.stream = _hip.current_stream_ptr(dev)

    def pick(self):
        g = self.g
        return float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # +-[0.1, 2]

    def row(self, n, absent, scale, zeta0, stream):
        row = _hip.StepRowC()
        for k in range(n):
            row.coef0[k] = (0.0 if k % 2 else -0.0) if k in absent else self.pick()  # an absent operand: an exact zero of either sign
        for k in range(_hip.ROW_TERMS):
            row.coef1[k] = NAN  # not read
        row.zeta0, row.stream0 = zeta0, stream
        row.chain, row.zeta1, row.stream1 = NAN, NAN, 99  # not read
        row.convert_k[0] = scale
        row.convert_k[1] = row.convert_k[2] = row.convert_k[3] = NAN  # not read
        return row

    def lone(self, b, row, n, slot, absent, noisy, store):
        "sample b alone through skr_step_launch_guided, with a plan that holds exactly the present operands in their order and the row's values"
        present = [k for k in range(n) if k not in absent]
        plan = make_plan(len(present), self.dtype, self.sn, noisy)
        for j, k in enumerate(present):
            plan.coef0[j] = row.coef0[k]
        plan.zeta0, plan.stream0 = row.zeta0, row.stream0
        out = torch.ones((1, self.sn), dtype=self.dtype, device=self.dev)
        guided = torch.ones((1, self.sn), dtype=self.dtype, device=self.dev) if store else None
        arr = (ctypes.c_void_p * len(present))(*[self.ops[k][b : b + 1].data_ptr() for k in present])
        guide = _hip.StepGuidanceC(self.cond[b : b + 1].data_ptr(), guided.data_ptr() if store else None, row.convert_k[0], present.index(slot), 0)
        rc = _hip.load().skr_step_launch_guided(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), self.seeds[b : b + 1].data_ptr(), self.sn, self.stream)
        assert rc == OK, rc
        return out[0], guided[0] if store else None

    def mixed(self, plan, ops, n, slot, store, table, index, row_offset):
        "(out, guided_out or None) of one rolling launch over all five samples, on outputs that hold the sentinel"
        out = self.sentinel.clone()
        guided = self.sentinel.clone() if store else None
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ops[:n]])
        guide = _hip.StepGuidanceC(self.cond.data_ptr(), guided.data_ptr() if store else None, 99.0, slot, 0)  # (guide->scale is ignored: a decoy)
        rc = _hip.load().skr_step_launch_guided_rolling(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), self.seeds.data_ptr(), SAMPLES * self.sn,
                                                        table.data_ptr(), index.data_ptr(), row_offset, self.stream)  # fmt: skip
        assert rc == OK, rc
        return out, guided


@pytest.mark.parametrize("sample_numel", [2048, 6144], ids=["one_chunk", "three_chunks"])  # a shift of 0, and the dividing branch of sample_of
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_mixed_launch_equals_the_lone_kernarg_launches(name, sample_numel, dev):
    """five samples at five places in one launch: each active one has, in `out` and in `guided_out`, the bits skr_step_launch_guided gives
    for it alone with the narrowed plan; the inactive one keeps its sentinel; also with guided_out == NULL and with a non-zero row_offset"""
    p = Problem(sample_numel, DTYPES[name], dev, seed=900 + sample_numel)
    for n in COUNTS:
        for slot in sorted({0, n // 2, n - 1}):
            absent = absent_sets(n, slot)
            if n >= 3:
                assert absent[2] and absent[3] and absent[2] != absent[3]
            ops = [t.clone() for t in p.ops[:n]]
            for b in (2, 3):
                for k in absent[b]:
                    ops[k][b].fill_(NAN)  # what an absent operand holds: never loaded
            for k in range(n):
                ops[k][0].fill_(NAN)  # the inactive sample: nothing of it is read ...
            # rows 1..4 of the samples 1..4; sample 4's zeta0 is zero: under a drawing launch it skips the draw
            rows = {b: p.row(n, absent[b], SCALES[b], 0.0 if b == 4 else 0.3 + 0.1 * b, (3 + b) * 256) for b in (1, 2, 3, 4)}
            for noisy in (False, True):
                plan = make_plan(n, p.dtype, p.sn, noisy)
                what = (name, sample_numel, n, slot, noisy)
                want = {b: p.lone(b, rows[b], n, slot, absent[b], noisy, True) for b in rows}
                quiet = {b: p.lone(b, rows[b], n, slot, absent[b], False, True) for b in rows}
                for b in rows:  # (the draw takes part exactly when the launch and the row say so)
                    assert torch.equal(bits(want[b][0]), bits(quiet[b][0])) != (noisy and b != 4), (what, b)
                    assert torch.isfinite(want[b][0].float()).all() and torch.isfinite(want[b][1].float()).all(), (what, b)
                table = upload([rows[1], junk_row(), rows[2], rows[3], junk_row(), rows[4]], dev)
                index = torch.tensor([-1, 0, 2, 3, 5], dtype=torch.int32, device=dev)
                runs = [("stored", True, table, index, 0)]
                if slot == n // 2:  # once per operand count: without guided_out, and through a row_offset (the -1 entry is tested before it is added)
                    shifted = upload([junk_row(), junk_row(), rows[1], junk_row(), rows[2], rows[3], junk_row(), rows[4]], dev)
                    runs += [("no guided_out", False, table, index, 0), ("row_offset", True, shifted, index, 2)]
                for label, store, tab, idx, offset in runs:
                    out, guided = p.mixed(decoy(plan), ops, n, slot, store, tab, idx, offset)
                    for b in rows:
                        assert torch.equal(bits(out[b]), bits(want[b][0])), (what, label, b, int((bits(out[b]) != bits(want[b][0])).sum()))
                        if store:
                            assert torch.equal(bits(guided[b]), bits(want[b][1])), (what, label, b)
                    assert torch.equal(bits(out[0]), bits(p.sentinel[0])), (what, label)  # ... and nothing of it is written
                    if store:
                        assert torch.equal(bits(guided[0]), bits(p.sentinel[0])), (what, label)


# ---- 2. the status table ---------------------------------------------------------------------------------------------------------------
def test_status_table_equals_the_per_sample_twin_and_nothing_is_written(dev):
    "for the same bad arguments the codes, and so their order (the two-fault rows), are skr_step_launch_guided_indexed_per_sample's"
    lib = _hip.load()
    numel, sn = 8192, 4096
    g = torch.Generator().manual_seed(800)
    a, b, cond = (torch.randn((2, sn), generator=g).bfloat16().to(dev) for _ in range(3))
    wide = [torch.randn((2, sn), generator=g).to(dev) for _ in range(3)]
    out, gout = torch.full_like(a, 7.0), torch.full_like(a, 7.0)
    out32, gout32 = torch.full_like(wide[0], 7.0), torch.full_like(wide[0], 7.0)
    seeds = torch.tensor([5, 6], dtype=torch.int64, device=dev)
    row = _hip.StepRowC()
    row.coef0[0], row.coef0[1], row.zeta0, row.stream0, row.convert_k[0] = 0.75, -0.5, 0.45, 512, 7.3
    table = upload([row, row], dev)
    index = torch.zeros(2, dtype=torch.int32, device=dev)

    def plan_of(**fields):
        plan = make_plan(2, torch.bfloat16, sn, True)
        for key, value in fields.items():
            setattr(plan, key, value)
        return plan

    def call(entry, plan=None, inputs=(a.data_ptr(), b.data_ptr()), out=out.data_ptr(), cond=cond.data_ptr(), gout=gout.data_ptr(), slot=1, reserved=0,
             seeds=seeds.data_ptr(), numel=numel, rows=table.data_ptr(), idx=index.data_ptr(), row_offset=0, no_plan=False, no_guide=False, no_inputs=False):  # fmt: skip
        plan = plan if plan is not None else plan_of()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
        return entry(None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide), seeds, numel, rows, idx, row_offset, None)

    only = dict(plan=plan_of(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a.data_ptr(),), slot=0)
    fp32 = dict(inputs=(wide[0].data_ptr(), wide[1].data_ptr()), cond=wide[2].data_ptr(), out=out32.data_ptr(), gout=gout32.data_ptr())
    cases = [
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("no rows", dict(rows=None), NULL),
        ("no sample index", dict(idx=None), NULL),
        ("a draw without seeds", dict(seeds=None), NULL),
        ("noise_mode 1 without seeds, whatever the plan's zeta0", dict(seeds=None, plan=plan_of(zeta0=0.0)), NULL),
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
        ("convert_from", dict(plan=plan_of(convert_from=2)), UNSUPPORTED),
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
        ("an out dtype outside the groups", dict(plan=plan_of(out0_dtype=_hip.F16)), DTYPE),
        # what the one-trip kernel does not cover: there is no grid-stride form
        ("a ragged numel", dict(numel=numel - 8, plan=plan_of(noise_mode=0)), UNSUPPORTED),
        ("a sample below a chunk under a draw", dict(numel=4096, plan=plan_of(sample_numel=1024)), UNSUPPORTED),
        ("two dtype groups", dict(plan=plan_of(n_group_a=1, dtype_b=_hip.F32)), UNSUPPORTED),
        ("an fp32 output of bf16 operands", dict(plan=plan_of(out0_dtype=_hip.F32)), UNSUPPORTED),
        ("fp64", dict(plan=plan_of(dtype_a=_hip.F64, out0_dtype=_hip.F64, acc_f64=1)), UNSUPPORTED),
        ("acc_f64", dict(plan=plan_of(acc_f64=1)), UNSUPPORTED),
        ("the guidance-only form", dict(only, out=None), UNSUPPORTED),
        ("a negative row_offset", dict(row_offset=-1), UNSUPPORTED),
        # a workgroup lies inside one sample, with or without noise
        ("no sample size without noise", dict(plan=plan_of(noise_mode=0, sample_numel=0)), SHAPE),
        ("samples that do not divide, without noise", dict(plan=plan_of(noise_mode=0, sample_numel=numel - 2048)), SHAPE),
        ("samples that do not divide, with noise", dict(plan=plan_of(sample_numel=numel - 2048)), SHAPE),
        ("a sample below a chunk without noise", dict(plan=plan_of(noise_mode=0, sample_numel=1024)), UNSUPPORTED),
        # two faults: the earlier check answers
        ("no rows + slot", dict(rows=None, slot=5), NULL),
        ("no sample index + slot", dict(idx=None, slot=5), NULL),
        ("no seeds + slot", dict(seeds=None, slot=5), NULL),
        ("slot + negative numel", dict(slot=2, numel=-1), TERMS),
        ("negative numel + reserved", dict(numel=-1, reserved=1), SHAPE),
        ("reserved + sample size", dict(reserved=1, plan=plan_of(sample_numel=4095)), UNSUPPORTED),
        ("sample size + no cond", dict(plan=plan_of(sample_numel=4095), cond=None), SHAPE),
        ("no cond + misaligned out", dict(cond=None, out=out.data_ptr() + 4), NULL),
        ("misaligned cond + dtype", dict(cond=cond.data_ptr() + 2, plan=plan_of(out0_dtype=_hip.F16)), ALIGN),
        ("dtype + a negative row_offset", dict(plan=plan_of(out0_dtype=_hip.F16), row_offset=-1), DTYPE),
        ("acc_f64 + a negative row_offset", dict(plan=plan_of(acc_f64=1), row_offset=-1), UNSUPPORTED),
        ("a negative row_offset + a sample below a chunk", dict(row_offset=-1, plan=plan_of(noise_mode=0, sample_numel=1024)), UNSUPPORTED),
    ]
    rolling_entry, twin = lib.skr_step_launch_guided_rolling, lib.skr_step_launch_guided_indexed_per_sample
    for what, kwargs, want in cases:
        assert call(rolling_entry, **kwargs) == call(twin, **kwargs) == want, what
    for key, tensors in ((b"one_trip", {}), (b"tile", fp32)):
        try:
            assert lib.skr_set_tuning(key, 0) == 0
            fields = dict(tensors, plan=plan_of(dtype_a=_hip.F32, out0_dtype=_hip.F32)) if tensors else {}
            assert call(rolling_entry, **fields) == call(twin, **fields) == UNSUPPORTED, key
        finally:
            lib.skr_set_tuning(key, 1)
    torch.cuda.synchronize()
    for t in (out, gout, out32, gout32):
        assert (t == 7.0).all()  # no refused launch wrote anything
    # a well-formed control: the plan's zeta0 is ignored (the row decides)
    for kwargs in ({}, dict(plan=plan_of(zeta0=0.0))):
        out.fill_(7.0), gout.fill_(7.0)
        assert call(rolling_entry, **kwargs) == OK, kwargs
        torch.cuda.synchronize()
        assert not (out == 7.0).all() and not (gout == 7.0).all()


# ---- guided rolling batches --------------------------------------------------------------------------------------------------------
W = PD.SkrampleWrapperScheduler
MAKERS = {
    "euler": lambda sch: W(PT.Euler(), sch),
    "dpm2": lambda sch: W(PT.DPM(order=2), sch),
    "dpm2_sde": lambda sch: W(PT.DPM(order=2, stochasticity=1.0), sch),
    "dpm3": lambda sch: W(PT.DPM(order=3), sch),
    "adams4": lambda sch: W(PT.Adams(order=4), sch),
    "unip3": lambda sch: W(PT.UniP(order=3), sch),
}
STOCHASTIC = ("dpm2_sde",)
UNIT, CAPACITY = (4, 16, 32), 3
# (tick of admission, slot, steps, schedule, seed, guidance): 3, 5 and 4 steps at ticks 0, 1 and 3; slot 0 is reused once its first
# request has left, slot 2 stays free throughout; a scale of one, a scale that is no fp32 value, and a schedule of distinct values
STAGGERED = [(0, 0, 3, 0, 11, 1.0), (1, 1, 5, 1, 12, 3.5), (3, 0, 4, 2, 13, (7.3, 5.1, -0.75, 2.0))]
COMMON = [(0, 0, 3, 0, 11, 3.3), (1, 1, 5, 1, 12, 3.3), (3, 0, 4, 2, 13, 3.3)]  # one common scale: what torch's three lines on the whole batch can do


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def net(x, t):
    "elementwise, two halves (uncond, cond), a pure per-sample function of (latents, timestep): `t` is one float32 per sample"
    s = (t.to(torch.float32) * (1.0 / 1024.0)).to(x.dtype).view(-1, *([1] * (x.dim() - 1)))
    return x * 0.25 + (s * 0.125) * x.abs(), x * 0.125 - 0.0625 * x.abs() + s * 0.25


def scales_of(guidance, steps):
    return list(guidance) if isinstance(guidance, tuple) else [guidance] * steps


def lone(kind, variant, steps, latents, seed, guidance):
    "the request alone: its own wrapper, batch 1, its own seed, step_guided with the scale of every step"
    w = MAKERS[kind](variants()[variant])
    w.set_timesteps(steps)
    x = latents.unsqueeze(0)
    for i, t in enumerate(w.timesteps.tolist()):
        uncond, cond = net(x, torch.tensor([t], dtype=torch.float32, device=x.device))
        x = w.step_guided(uncond, cond, scales_of(guidance, steps)[i], t, x, generator=[seed] if kind in STOCHASTIC else None, return_dict=False)[0]
    return x[0].clone()


@functools.lru_cache(maxsize=None)
def yardstick(kind, dtype, common=False):
    "(requests, lone results), computed once per case and shared, never written to.  requests: [(tick, slot, steps, variant, seed, guidance, latents)]"
    td, dev, g = DTYPES[dtype], torch.device("cuda:0"), torch.Generator().manual_seed(17)
    requests = [(*entry, torch.randn(UNIT, generator=g).to(td).to(dev)) for entry in (COMMON if common else STAGGERED)]
    refs = [lone(kind, variant, steps, latents, seed, guidance) for _, _, steps, variant, seed, guidance, latents in requests]
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs)
    return requests, refs


def serve(batch, kind, requests, tick, guided=True):
    "admits each request at its tick and calls `tick()` (-> finished slots) until all are done: {request number: result}"
    results, resident, at_tick = {}, {}, 0
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, seed, guidance, latents) in enumerate(requests):
            if at == at_tick:
                extra = dict(guidance_scale=list(guidance) if isinstance(guidance, tuple) else guidance) if guided else {}
                batch.admit(slot, latents, MAKERS[kind](variants()[variant]), steps, seed=seed if kind in STOCHASTIC else None, **extra)
                resident[slot] = n
        assert batch.active
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        at_tick += 1
        assert at_tick < 32
    torch.cuda.synchronize()
    return results


def make_batch(kind, dtype, dev, **options):
    example = torch.zeros((CAPACITY, *UNIT), dtype=DTYPES[dtype], device=dev)
    return RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=CAPACITY, **options)


def host_tick(batch):
    return lambda: batch.step_guided(*net(batch.latents, batch.timesteps))


def check_against(results, refs, what):
    assert len(results) == len(refs)
    for n, ref in enumerate(refs):
        assert torch.equal(bits(results[n]), bits(ref)), (*what, n, int((bits(results[n]) != bits(ref)).sum()))


CASES = [(kind, dtype) for kind in sorted(MAKERS) for dtype in ("bf16", "fp16")] + [("dpm2_sde", "fp32")]


@pytest.mark.parametrize("kind,dtype", CASES)
def test_staggered_requests_equal_their_lone_runs(kind, dtype, dev):
    "3 requests of 3, 5 and 4 steps, admitted at ticks 0, 1 and 3 under a scale of 1, a scale of 3.5 and a guidance schedule: one launch a tick"
    requests, refs = yardstick(kind, dtype)
    batch = make_batch(kind, dtype, dev, guided=True)
    assert batch.guided and batch.roles[batch.slot] == ("o",) and len(batch._g) == (batch.keep + 2 if batch.keep else 0)
    check_against(serve(batch, kind, requests, host_tick(batch)), refs, (kind, dtype))
    assert not batch.active and batch._outputs == [] and batch._stamps == []  # nothing of the caller was held
    assert not torch.equal(refs[0], refs[1])


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams4"])
def test_the_unfused_route_gives_the_same_bits(kind, dev):
    "torch's three lines on the whole batch with one common scale, handed to a plain RollingBatch.step(): the guided batch's results"
    requests, refs = yardstick(kind, "bf16", common=True)
    guided = make_batch(kind, "bf16", dev, guided=True)
    fused = serve(guided, kind, requests, host_tick(guided))
    check_against(fused, refs, (kind, "fused"))
    plain = make_batch(kind, "bf16", dev)

    def three_lines():
        uncond, cond = net(plain.latents, plain.timesteps)
        return plain.step(uncond + 3.3 * (cond - uncond))

    check_against(serve(plain, kind, requests, three_lines, guided=False), [fused[n] for n in range(len(requests))], (kind, "three lines"))


def test_a_poisoned_slot_does_not_reach_an_admitted_request(dev):
    "every ring tensor's slice of a free slot holds NaN -- what a previous occupant may have left: the request admitted into it equals its lone run"
    kind = "adams4"
    requests, refs = yardstick(kind, "bf16")
    batch = make_batch(kind, "bf16", dev, guided=True)
    assert len(batch._g) == 5 and all(any(t is r for r in batch.ring_tensors()) for t in batch._g)
    for t in batch.ring_tensors():
        t[1].fill_(NAN)
    _, slot, steps, variant, seed, guidance, latents = requests[1]
    assert slot == 1
    batch.admit(slot, latents, MAKERS[kind](variants()[variant]), steps, guidance_scale=guidance)
    tick, done = host_tick(batch), []
    while not done:
        done = tick()
    assert torch.equal(bits(batch.take(1)), bits(refs[1]))


def test_the_same_prediction_in_both_halves_is_the_plain_run(dev):
    "an unguided request sharing a guided batch: cond - uncond is exactly 0, so it equals the plain rolling run whatever its scale"
    kind = "dpm2_sde"
    requests, _ = yardstick(kind, "bf16")
    plain = make_batch(kind, "bf16", dev)
    expected = serve(plain, kind, requests, lambda: plain.step(net(plain.latents, plain.timesteps)[0]), guided=False)
    guided = make_batch(kind, "bf16", dev, guided=True)

    def tick():
        uncond = net(guided.latents, guided.timesteps)[0]
        return guided.step_guided(uncond, uncond.clone())

    check_against(serve(guided, kind, requests, tick), [expected[n] for n in range(len(requests))], (kind,))


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams4"])
def test_device_positions_and_captured_ticks_equal_the_host_published_run(kind, dev):
    requests, refs = yardstick(kind, "bf16")
    eager = make_batch(kind, "bf16", dev, guided=True, device_positions=True)

    def device_tick():
        eager.advance()
        return eager.step_guided(*net(eager.latents, eager.timesteps))

    check_against(serve(eager, kind, requests, device_tick), refs, (kind, "advance"))
    batch = make_batch(kind, "bf16", dev, guided=True, device_positions=True)
    ticks = batch.capture(net)
    assert ticks.phases == batch.keep + 2 == len(ticks.graphs) == len(ticks.outputs) == len(ticks.conds)
    check_against(serve(batch, kind, requests, ticks.tick), refs, (kind, "captured"))
    assert ticks.ticks > ticks.phases and min(ticks.replays) >= 1
    with pytest.raises(ValueError, match="captured"):
        batch.step_guided(*net(batch.latents, batch.timesteps))


def test_refusals_name_their_reason_and_upload_nothing(dev, monkeypatch):
    uploads = []
    held = rolling.upload_rows
    monkeypatch.setattr(rolling, "upload_rows", lambda *args: (uploads.append(args), held(*args)))
    example = torch.zeros((CAPACITY, *UNIT), dtype=torch.bfloat16, device=dev)
    sch = PS.Scaled
    before = torch.cuda.memory_allocated(dev)
    for sampler, says in ((PT.UniPC(order=2), "UniPC"), (PT.SPC(), "SPC")):
        with pytest.raises(_hip.SkrampleHipError, match=f"{says} is not one fused launch"):
            RollingBatch(lambda: W(sampler, sch()), example, capacity=CAPACITY, guided=True)
    with pytest.raises(_hip.SkrampleHipError, match="compute_scale=None is not one fused launch"):
        RollingBatch(lambda: W(PT.DPM(order=2), sch(), compute_scale=None), example, capacity=CAPACITY, guided=True)
    with pytest.raises(ValueError, match="guided together with inpaint_mask_shape"):
        RollingBatch(lambda: W(PT.DPM(order=2), sch()), example, capacity=CAPACITY, guided=True, inpaint_mask_shape=(1, 16, 32))
    with pytest.raises(ValueError, match="guided together with Offset noise"):
        RollingBatch(lambda: W(PT.DPM(order=2, stochasticity=1.0), sch(), noise_type=generators.Offset), example, capacity=CAPACITY, guided=True)
    assert torch.cuda.memory_allocated(dev) == before  # refused before a ring, a table or a dry run
    guided, plain = make_batch("dpm2", "bf16", dev, guided=True), make_batch("dpm2", "bf16", dev)
    x = torch.zeros(UNIT, dtype=torch.bfloat16, device=dev)
    out = torch.zeros((CAPACITY, *UNIT), dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="guidance_scale is required on a guided batch"):
        guided.admit(0, x, MAKERS["dpm2"](sch()), 4)
    with pytest.raises(ValueError, match="one scale per step: 3 scales for 4 steps"):
        guided.admit(0, x, MAKERS["dpm2"](sch()), 4, guidance_scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="needs a batch built with guided=True"):
        plain.admit(0, x, MAKERS["dpm2"](sch()), 4, guidance_scale=2.0)
    assert uploads == [] and guided.free(0) and plain.free(0) and not guided.rows_dev.any() and not plain.rows_dev.any()
    guided.admit(0, x, MAKERS["dpm2"](sch()), 4, guidance_scale=2.0)
    plain.admit(0, x, MAKERS["dpm2"](sch()), 4)
    ticks = (guided.ticks, plain.ticks)
    with pytest.raises(ValueError, match="step_guided"):
        guided.step(out)
    with pytest.raises(ValueError, match="guided=True"):
        plain.step_guided(out, out)
    with pytest.raises(ValueError, match="cond of a tick is a contiguous"):
        guided.step_guided(out, out.float())
    assert (guided.ticks, plain.ticks) == ticks and len(uploads) == 2 and guided.index_dev.tolist() == [-1] * CAPACITY
