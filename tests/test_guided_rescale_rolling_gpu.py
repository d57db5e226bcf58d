"""Rescaled guidance in rolling batches (needs an MI355X): skr_guidance_rescale_factor_rolling and skr_step_launch_guided_rescaled_rolling
through the C ABI, and `RollingBatch(guided=True, rescaled=True)` -- a guidance scale and a guidance_rescale per request, or per step, two
launches a tick.

The yardstick of every test is code that existed before the two entries: skr_guidance_rescale_factor and skr_step_launch_guided_rescaled
(or, for a sample that does not rescale, skr_step_launch_guided) on one sample alone with the narrowed plan, the eager
`step_guided(..., guidance_rescale=phi)` run of a lone wrapper, a guided batch built without `rescaled`, and the status codes of
skr_step_launch_guided_rolling and skr_guidance_rescale_factor.  Every comparison is therefore bitwise; there is no tolerance to choose.
Every index handed to a kernel names a row of its table."""

import ctypes
import functools

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
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
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


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


def lone_factor(u, c, scale, dev, stats=False):
    "(factor T[1], stats double[2] or None, partials) of skr_guidance_rescale_factor on one sample alone"
    sn = u.numel()
    factor = torch.zeros(1, dtype=u.dtype, device=dev)
    both = torch.zeros(2, dtype=torch.float64, device=dev) if stats else None
    partials = torch.zeros(_hip.guidance_partials(sn, sn), dtype=torch.float64, device=dev)
    rc = _hip.load().skr_guidance_rescale_factor(u.data_ptr(), c.data_ptr(), _hip.DTYPE_CODE[u.dtype], scale, sn, sn, factor.data_ptr(), both.data_ptr() if stats else None,
                                                 partials.data_ptr(), _hip.current_stream_ptr(dev))  # fmt: skip
    assert rc == OK, rc
    return factor, both, partials


# ---- 1. the statistics entry through the C ABI -----------------------------------------------------------------------------------------
# six samples: 0 inactive (NaN in uncond and cond), 1..3 active and rescaled (2: mean 100, std 0.01 -- the pivot), 4: phi = 0.0, 5: phi = -0.0
STAT_SCALES = [NAN, 7.3, -2.6, 3.3, 5.0, 5.0]
STAT_PHIS = [NAN, 0.7, 1.0, 0.25, 0.0, -0.0]
SENTINEL = 123.0


def stat_row(scale, phi):
    "what the statistics launch reads of a row: convert_k[0] and convert_k[1]; everything else a NaN"
    row = junk_row()
    row.convert_k[0], row.convert_k[1] = scale, phi
    return row


@pytest.mark.parametrize("sample_numel", [2048, 6144], ids=["one_span", "three_spans"])  # stage 2 sums one partial / its order matters
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_rolling_factor_equals_the_lone_statistics_launch(name, sample_numel, dev):
    dtype, sn = DTYPES[name], sample_numel
    g = torch.Generator().manual_seed(300 + sn)
    u = torch.randn((6, sn), generator=g).to(dtype).to(dev)
    c = torch.randn((6, sn), generator=g).to(dtype).to(dev)
    u[2] = (100.0 + 0.01 * torch.randn(sn, generator=g)).to(dtype).to(dev)
    c[2] = (100.0 + 0.01 * torch.randn(sn, generator=g)).to(dtype).to(dev)
    u[0].fill_(NAN), c[0].fill_(NAN)
    rows = {s: stat_row(STAT_SCALES[s], STAT_PHIS[s]) for s in range(1, 6)}
    want = {s: lone_factor(u[s], c[s], STAT_SCALES[s], dev, stats=True) for s in (1, 2, 3)}
    spans = sn // 2048
    table = upload([rows[1], junk_row(), rows[2], rows[3], junk_row(), rows[4], junk_row(), rows[5]], dev)
    shifted = upload([junk_row(), junk_row(), rows[1], junk_row(), rows[2], rows[3], junk_row(), rows[4], junk_row(), rows[5]], dev)
    index = torch.tensor([-1, 0, 2, 3, 5, 7], dtype=torch.int32, device=dev)
    for label, tab, offset, with_stats in (("stats", table, 0, True), ("no stats", table, 0, False), ("row_offset", shifted, 2, True)):
        factor = torch.full((6,), SENTINEL, dtype=dtype, device=dev)
        stats = torch.full((12,), SENTINEL, dtype=torch.float64, device=dev)
        partials = torch.full((_hip.guidance_partials(6 * sn, sn),), NAN, dtype=torch.float64, device=dev)
        rc = _hip.load().skr_guidance_rescale_factor_rolling(u.data_ptr(), c.data_ptr(), _hip.DTYPE_CODE[dtype], 6 * sn, sn, tab.data_ptr(), index.data_ptr(), offset,
                                                             factor.data_ptr(), stats.data_ptr() if with_stats else None, partials.data_ptr(), _hip.current_stream_ptr(dev))  # fmt: skip
        assert rc == OK, (label, rc)
        torch.cuda.synchronize()
        what = (name, sn, label)
        for s, (f, both, parts) in want.items():
            print(what, s, float(f[0]), both.tolist(), float(factor[s]))
            assert torch.equal(bits(factor[s : s + 1]), bits(f)), (what, s, float(factor[s]), float(f[0]))
            assert torch.equal(bits(partials[4 * spans * s : 4 * spans * (s + 1)]), bits(parts)), (what, s)  # the partials layout, unchanged
            if with_stats:
                assert torch.equal(bits(stats[2 * s : 2 * s + 2]), bits(both)), (what, s)
        assert want[2][1][0] < 0.1 or dtype != torch.float32  # (the pivot sample is one: a std far below its mean)
        for s in (0, 4, 5):  # inactive, phi = 0.0, phi = -0.0: nothing written
            assert float(factor[s]) == SENTINEL and (stats[2 * s : 2 * s + 2] == SENTINEL).all(), (what, s)
            assert torch.isnan(partials[4 * spans * s : 4 * spans * (s + 1)]).all(), (what, s)
        if not with_stats:
            assert (stats == SENTINEL).all(), what


# ---- 2. the step entry through the C ABI -----------------------------------------------------------------------------------------------
SAMPLES = 6  # 0: inactive, 1: every operand, 2 and 3: two subsets absent (their bytes NaN), 4: zeta0 == 0, 5: phi == 0 (its factor NaN)
COUNTS = (1, 2, 3, 4, 5, 8, 9, 16)  # every guided_kmax bucket and its edges
SCALES = [NAN, 7.3, -2.6, 1.0, 3.3, 2.2]  # per sample; neither 7.3 nor 3.3 is an fp32 value, one scale is negative
PHIS = [NAN, 0.7, 1.0, 0.25, 0.7, 0.0]  # 0.7 is no fp32 value; 1.0: psi = 0


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


def absent_sets(n, slot):
    "the operands sample 2 and sample 3 do not have: two different subsets of the operands other than `slot` (empty when there is no other)"
    others = [k for k in range(n) if k != slot]
    return {1: [], 2: others[0::2], 3: others[1::2] if len(others) > 1 else others, 4: [], 5: []}


class Problem:
    "the tensors of one sample size and dtype (16 operands: a launch of n takes the first n), shared by every case of a test and never written"

    def __init__(self, sample_numel, dtype, dev, seed):
        self.shape, self.dtype, self.dev, self.sn = (SAMPLES, sample_numel), dtype, dev, sample_numel
        self.g = g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(self.shape, generator=g).to(dtype).to(dev) for _ in range(_hip.ROW_TERMS)]
        self.cond = torch.randn(self.shape, generator=g).to(dtype).to(dev)
        self.cond[0].fill_(NAN)  # the inactive sample: nothing of it is read
        self.seeds = torch.tensor([11, 22, 33, 44, 55, 66], dtype=torch.int64, device=dev)
        self.sentinel = (torch.arange(SAMPLES * sample_numel, device=dev) % 251).reshape(self.shape).to(dtype)
        self.partials = torch.zeros(_hip.guidance_partials(SAMPLES * sample_numel, sample_numel), dtype=torch.float64, device=dev)
        self.stream = _hip.current_stream_ptr(dev)

    def pick(self):
        g = self.g
        return float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # +-[0.1, 2]

    def row(self, n, absent, scale, phi, zeta0, stream):
        row = _hip.StepRowC()
        for k in range(n):
            row.coef0[k] = (0.0 if k % 2 else -0.0) if k in absent else self.pick()  # an absent operand: an exact zero of either sign
        for k in range(_hip.ROW_TERMS):
            row.coef1[k] = NAN  # not read
        row.zeta0, row.stream0 = zeta0, stream
        row.chain, row.zeta1, row.stream1 = NAN, NAN, 99  # not read
        row.convert_k[0], row.convert_k[1] = scale, phi
        row.convert_k[2] = row.convert_k[3] = NAN  # not read
        return row

    def lone(self, b, row, n, slot, absent, noisy, store):
        """sample b alone, with a plan that holds exactly the present operands in their order and the row's values: through
        skr_guidance_rescale_factor and skr_step_launch_guided_rescaled when its phi is not zero, through skr_step_launch_guided when it is.
        (out, guided_out or None, factor or None)"""
        present = [k for k in range(n) if k not in absent]
        plan = make_plan(len(present), self.dtype, self.sn, noisy)
        for j, k in enumerate(present):
            plan.coef0[j] = row.coef0[k]
        plan.zeta0, plan.stream0 = row.zeta0, row.stream0
        out = torch.ones((1, self.sn), dtype=self.dtype, device=self.dev)
        guided = torch.ones((1, self.sn), dtype=self.dtype, device=self.dev) if store else None
        arr = (ctypes.c_void_p * len(present))(*[self.ops[k][b : b + 1].data_ptr() for k in present])
        guide = _hip.StepGuidanceC(self.cond[b : b + 1].data_ptr(), guided.data_ptr() if store else None, row.convert_k[0], present.index(slot), 0)
        lib, seeds, factor = _hip.load(), self.seeds[b : b + 1].data_ptr(), None
        if row.convert_k[1] == 0.0:
            rc = lib.skr_step_launch_guided(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), seeds, self.sn, self.stream)
        else:
            factor, _, _ = lone_factor(self.ops[slot][b], self.cond[b], row.convert_k[0], self.dev)
            rescale = _hip.StepRescaleC(factor.data_ptr(), row.convert_k[1], self.sn, 0)
            rc = lib.skr_step_launch_guided_rescaled(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(rescale), seeds, self.sn, self.stream)
        assert rc == OK, rc
        return out[0], guided[0] if store else None, factor

    def mixed(self, plan, ops, n, slot, store, table, index, row_offset):
        "(out, guided_out or None, factor) of the two rolling launches over all six samples, on outputs that hold the sentinel and factors that hold NaN"
        out = self.sentinel.clone()
        guided = self.sentinel.clone() if store else None
        factor = torch.full((SAMPLES,), NAN, dtype=self.dtype, device=self.dev)
        self.partials.fill_(NAN)
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ops[:n]])
        lib, numel = _hip.load(), SAMPLES * self.sn
        rc = lib.skr_guidance_rescale_factor_rolling(ops[slot].data_ptr(), self.cond.data_ptr(), _hip.DTYPE_CODE[self.dtype], numel, self.sn, table.data_ptr(), index.data_ptr(),
                                                     row_offset, factor.data_ptr(), None, self.partials.data_ptr(), self.stream)  # fmt: skip
        assert rc == OK, rc
        guide = _hip.StepGuidanceC(self.cond.data_ptr(), guided.data_ptr() if store else None, 99.0, slot, 0)  # (guide->scale is ignored: a decoy)
        rescale = _hip.StepRescaleC(factor.data_ptr(), 0.33, self.sn, 0)  # (rescale->phi is ignored: a decoy)
        rc = lib.skr_step_launch_guided_rescaled_rolling(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(rescale), self.seeds.data_ptr(), numel,
                                                         table.data_ptr(), index.data_ptr(), row_offset, self.stream)  # fmt: skip
        assert rc == OK, rc
        return out, guided, factor


@pytest.mark.parametrize("sample_numel", [2048, 6144], ids=["one_chunk", "three_chunks"])  # a shift of 0, and the dividing branch of sample_of
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_mixed_launch_equals_the_lone_rescaled_launches(name, sample_numel, dev):
    """six samples at six places in the two launches: each active one has, in `out` and in `guided_out`, the bits the lone entries give it
    alone with the narrowed plan; the one whose phi is zero those of skr_step_launch_guided, under a factor that stays NaN; the inactive one
    keeps its sentinel; also with guided_out == NULL and with a non-zero row_offset"""
    p = Problem(sample_numel, DTYPES[name], dev, seed=700 + sample_numel)
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
            phis = list(PHIS)
            phis[5] = 0.0 if n % 2 else -0.0  # either sign of zero
            # rows 1..5 of the samples 1..5; sample 4's zeta0 is zero: under a drawing launch it skips the draw
            rows = {b: p.row(n, absent[b], SCALES[b], phis[b], 0.0 if b == 4 else 0.3 + 0.1 * b, (3 + b) * 256) for b in range(1, SAMPLES)}
            for noisy in (False, True):
                plan = make_plan(n, p.dtype, p.sn, noisy)
                what = (name, sample_numel, n, slot, noisy)
                want = {b: p.lone(b, rows[b], n, slot, absent[b], noisy, True) for b in rows}
                for b in rows:
                    assert torch.isfinite(want[b][0].float()).all() and torch.isfinite(want[b][1].float()).all(), (what, b)
                table = upload([rows[1], junk_row(), rows[2], rows[3], junk_row(), rows[4], rows[5]], dev)
                index = torch.tensor([-1, 0, 2, 3, 5, 6], dtype=torch.int32, device=dev)
                runs = [("stored", True, table, index, 0)]
                if slot == n // 2:  # once per operand count: without guided_out, and through a row_offset (the -1 entry is tested before it is added)
                    shifted = upload([junk_row(), junk_row(), rows[1], junk_row(), rows[2], rows[3], junk_row(), rows[4], rows[5]], dev)
                    runs += [("no guided_out", False, table, index, 0), ("row_offset", True, shifted, index, 2)]
                for label, store, tab, idx, offset in runs:
                    out, guided, factor = p.mixed(decoy(plan), ops, n, slot, store, tab, idx, offset)
                    for b in rows:
                        assert torch.equal(bits(out[b]), bits(want[b][0])), (what, label, b, int((bits(out[b]) != bits(want[b][0])).sum()))
                        if store:
                            assert torch.equal(bits(guided[b]), bits(want[b][1])), (what, label, b)
                        if want[b][2] is not None:
                            assert torch.equal(bits(factor[b : b + 1]), bits(want[b][2])), (what, label, b)
                    assert torch.isnan(factor[0]) and torch.isnan(factor[5]), (what, label)  # never written -- and, for sample 5, never read
                    assert torch.equal(bits(out[0]), bits(p.sentinel[0])), (what, label)  # ... and nothing of it is written
                    if store:
                        assert torch.equal(bits(guided[0]), bits(p.sentinel[0])), (what, label)


def test_a_rescaled_sample_differs_from_its_unrescaled_self_and_psi_zero_is_the_rescaled_prediction(dev):
    "the yardsticks are not vacuous: phi = 0.7 moves the result off the unrescaled launch's, and at phi = 1.0 guided_out is rn(1.0 * rn(p * r)) + rn(0 * p)"
    p = Problem(2048, torch.bfloat16, dev, seed=77)
    n, slot = 3, 1
    rows = {b: p.row(n, [], SCALES[b], PHIS[b], 0.0, 256) for b in range(1, SAMPLES)}
    table = upload([rows[b] for b in range(1, SAMPLES)], dev)
    index = torch.tensor([-1, 0, 1, 2, 3, 4], dtype=torch.int32, device=dev)
    out, guided, factor = p.mixed(make_plan(n, p.dtype, p.sn, False), p.ops, n, slot, True, table, index, 0)
    plain_out, plain_guided = p.sentinel.clone(), p.sentinel.clone()
    arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in p.ops[:n]])
    guide = _hip.StepGuidanceC(p.cond.data_ptr(), plain_guided.data_ptr(), 0.0, slot, 0)
    rc = _hip.load().skr_step_launch_guided_rolling(ctypes.byref(make_plan(n, p.dtype, p.sn, False)), arr, plain_out.data_ptr(), ctypes.byref(guide), None, SAMPLES * p.sn,
                                                    table.data_ptr(), index.data_ptr(), 0, p.stream)  # fmt: skip
    assert rc == OK
    for b in (1, 2, 4):  # (sample 3's scale is 1.0: its p is cond up to rounding, and its factor may round to 1)
        assert not torch.equal(bits(guided[b]), bits(plain_guided[b])), b
    assert torch.equal(bits(guided[5]), bits(plain_guided[5])) and torch.equal(bits(out[5]), bits(plain_out[5]))  # phi == 0: the unrescaled launch's bits
    resc = (plain_guided[2] * factor[2]) * 1.0 + 0.0 * plain_guided[2]  # torch's own ops on bf16 tensors, phi = 1.0
    assert torch.equal(bits(guided[2]), bits(resc))


# ---- 3. the status tables ---------------------------------------------------------------------------------------------------------------
def test_status_tables_equal_their_yardsticks_and_nothing_is_written(dev):
    """every code of the two entries in its stated order, two-fault rows included: the step entry answers what skr_step_launch_guided_rolling
    answers where the arguments are the twin's, the statistics entry what skr_guidance_rescale_factor answers where the checks are its own"""
    lib = _hip.load()
    numel, sn = 8192, 4096
    g = torch.Generator().manual_seed(800)
    a, b, cond = (torch.randn((2, sn), generator=g).bfloat16().to(dev) for _ in range(3))
    out, gout = torch.full_like(a, 7.0), torch.full_like(a, 7.0)
    factor = torch.full((2,), 7.0, dtype=torch.bfloat16, device=dev)
    stats = torch.full((4,), 7.0, dtype=torch.float64, device=dev)
    partials = torch.full((_hip.guidance_partials(numel, sn),), 7.0, dtype=torch.float64, device=dev)
    seeds = torch.tensor([5, 6], dtype=torch.int64, device=dev)
    row = _hip.StepRowC()
    row.coef0[0], row.coef0[1], row.zeta0, row.stream0, row.convert_k[0], row.convert_k[1] = 0.75, -0.5, 0.45, 512, 7.3, 0.7
    table = upload([row, row], dev)
    index = torch.zeros(2, dtype=torch.int32, device=dev)

    def plan_of(**fields):
        plan = make_plan(2, torch.bfloat16, sn, True)
        for key, value in fields.items():
            setattr(plan, key, value)
        return plan

    twin = lib.skr_step_launch_guided_rolling

    def step(entry, plan=None, inputs=(a.data_ptr(), b.data_ptr()), out=out.data_ptr(), cond=cond.data_ptr(), gout=gout.data_ptr(), slot=1, reserved=0, seeds=seeds.data_ptr(),
             numel=numel, rows=table.data_ptr(), idx=index.data_ptr(), row_offset=0, no_plan=False, no_guide=False, no_inputs=False, no_rescale=False,
             factor=factor.data_ptr(), rs_numel=None, rs_reserved=0):  # fmt: skip
        plan = plan if plan is not None else plan_of()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
        head = (None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide))
        if entry is twin:
            return entry(*head, seeds, numel, rows, idx, row_offset, None)
        rescale = _hip.StepRescaleC(factor, 0.25, plan.sample_numel if rs_numel is None else rs_numel, rs_reserved)
        return entry(*head, None if no_rescale else ctypes.byref(rescale), seeds, numel, rows, idx, row_offset, None)

    only = dict(plan=plan_of(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a.data_ptr(),), slot=0)
    shared = [  # the twin's arguments (the statistic's sample follows the plan's)
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("no rows", dict(rows=None), NULL),
        ("no sample index", dict(idx=None), NULL),
        ("a draw without seeds", dict(seeds=None), NULL),
        ("too many operands", dict(plan=plan_of(n_terms=17, n_group_a=17)), TERMS),
        ("slot beyond the operands", dict(slot=2), TERMS),
        ("negative numel", dict(numel=-8), SHAPE),
        ("noise_mode 2", dict(plan=plan_of(noise_mode=2)), UNSUPPORTED),
        ("a second output", dict(plan=plan_of(out1_dtype=_hip.BF16)), UNSUPPORTED),
        ("convert_to", dict(plan=plan_of(convert_to=1)), UNSUPPORTED),
        ("reserved", dict(reserved=1), UNSUPPORTED),
        ("guidance-only with an out pointer", dict(only), UNSUPPORTED),
        ("samples that do not divide the launch", dict(plan=plan_of(sample_numel=4095)), SHAPE),
        ("no inputs", dict(no_inputs=True), NULL),
        ("no out", dict(out=None), NULL),
        ("no cond", dict(cond=None), NULL),
        ("a NULL operand", dict(inputs=(a.data_ptr(), None)), NULL),
        ("a misaligned operand", dict(inputs=(a.data_ptr(), b.data_ptr() + 2)), ALIGN),
        ("a misaligned out", dict(out=out.data_ptr() + 4), ALIGN),
        ("a misaligned guided_out", dict(gout=gout.data_ptr() + 8), ALIGN),
        ("an out dtype outside the groups", dict(plan=plan_of(out0_dtype=_hip.F16)), DTYPE),
        ("a ragged numel", dict(numel=numel - 8, plan=plan_of(noise_mode=0, sample_numel=8)), UNSUPPORTED),
        ("two dtype groups", dict(plan=plan_of(n_group_a=1, dtype_b=_hip.F32)), UNSUPPORTED),
        ("acc_f64", dict(plan=plan_of(acc_f64=1)), UNSUPPORTED),
        ("a negative row_offset", dict(row_offset=-1), UNSUPPORTED),
        ("samples that do not divide, without noise", dict(plan=plan_of(noise_mode=0, sample_numel=numel - 2048), rs_numel=sn), SHAPE),
        ("a sample below a chunk without noise", dict(plan=plan_of(noise_mode=0, sample_numel=1024)), UNSUPPORTED),
        ("no rows + slot", dict(rows=None, slot=5), NULL),
        ("slot + negative numel", dict(slot=2, numel=-1), TERMS),
        ("negative numel + reserved", dict(numel=-1, reserved=1), SHAPE),
        ("no cond + misaligned out", dict(cond=None, out=out.data_ptr() + 4), NULL),
        ("misaligned cond + dtype", dict(cond=cond.data_ptr() + 2, plan=plan_of(out0_dtype=_hip.F16)), ALIGN),
        ("dtype + a negative row_offset", dict(plan=plan_of(out0_dtype=_hip.F16), row_offset=-1), DTYPE),
    ]
    entry = lib.skr_step_launch_guided_rescaled_rolling
    for what, kwargs, want in shared:
        twin_kwargs = {k: v for k, v in kwargs.items() if k != "rs_numel"}
        assert step(entry, **kwargs) == step(twin, **twin_kwargs) == want, what
    own = [  # what the rescale descriptor adds
        ("no rescale", dict(no_rescale=True), NULL),
        ("no rescale + slot", dict(no_rescale=True, slot=5), NULL),
        ("rescale reserved", dict(rs_reserved=1), UNSUPPORTED),
        ("negative numel + rescale reserved", dict(numel=-1, rs_reserved=1), SHAPE),
        ("rescale reserved + another sample", dict(rs_reserved=1, rs_numel=2048), UNSUPPORTED),
        ("another sample", dict(rs_numel=2048), SHAPE),
        ("another sample, without noise", dict(rs_numel=2048, plan=plan_of(noise_mode=0)), SHAPE),
        ("another sample + no factor", dict(rs_numel=2048, factor=None), SHAPE),
        ("no factor", dict(factor=None), NULL),
        ("no factor + misaligned out", dict(factor=None, out=out.data_ptr() + 4), NULL),
        ("no factor + a negative row_offset", dict(factor=None, row_offset=-1), NULL),
    ]
    for what, kwargs, want in own:
        assert step(entry, **kwargs) == want, what

    lone = lib.skr_guidance_rescale_factor

    def stat(rolling_entry, uncond=a.data_ptr(), cond=cond.data_ptr(), dtype=_hip.BF16, numel=numel, sample_numel=sn, rows=table.data_ptr(), idx=index.data_ptr(), row_offset=0,
             factor=factor.data_ptr(), partials=partials.data_ptr()):  # fmt: skip
        if rolling_entry:
            return lib.skr_guidance_rescale_factor_rolling(uncond, cond, dtype, numel, sample_numel, rows, idx, row_offset, factor, stats.data_ptr(), partials, None)
        return lone(uncond, cond, dtype, 7.3, numel, sample_numel, factor, stats.data_ptr(), partials, None)

    for what, kwargs, want in [  # the checks of skr_guidance_rescale_factor: its codes, its order
        ("no uncond", dict(uncond=None), NULL),
        ("no cond", dict(cond=None), NULL),
        ("no factor", dict(factor=None), NULL),
        ("no partials", dict(partials=None), NULL),
        ("no partials + negative numel", dict(partials=None, numel=-1), NULL),
        ("negative numel", dict(numel=-1), SHAPE),
        ("a sample of one element", dict(sample_numel=1), SHAPE),
        ("samples that do not divide", dict(sample_numel=6144), SHAPE),
        ("negative numel + misaligned uncond", dict(numel=-1, uncond=a.data_ptr() + 2), SHAPE),
        ("an empty launch", dict(numel=0), OK),
        ("an empty launch + misaligned cond + dtype", dict(numel=0, cond=cond.data_ptr() + 2, dtype=99), OK),
        ("misaligned uncond", dict(uncond=a.data_ptr() + 2), ALIGN),
        ("misaligned cond + dtype", dict(cond=cond.data_ptr() + 4, dtype=99), ALIGN),
        ("no tensor dtype", dict(dtype=99), DTYPE),
    ]:
        assert stat(True, **kwargs) == stat(False, **{k: v for k, v in kwargs.items()}) == want, what
    for what, kwargs, want in [  # what the rolling entry adds
        ("no rows", dict(rows=None), NULL),
        ("no sample index", dict(idx=None), NULL),
        ("no sample index + negative numel", dict(idx=None, numel=-1), NULL),
        ("dtype + a negative row_offset", dict(dtype=99, row_offset=-1), DTYPE),
        ("misaligned uncond + fp64", dict(uncond=a.data_ptr() + 2, dtype=_hip.F64), ALIGN),
        ("fp64", dict(dtype=_hip.F64), UNSUPPORTED),
        ("samples of no whole spans", dict(numel=6000, sample_numel=3000), UNSUPPORTED),
        ("samples below a span", dict(sample_numel=1024), UNSUPPORTED),
        ("a negative row_offset", dict(row_offset=-1), UNSUPPORTED),
        ("more than INT32_MAX spans", dict(numel=4096 * ((1 << 30) + 1), sample_numel=4096), UNSUPPORTED),
    ]:
        assert stat(True, **kwargs) == want, what
    torch.cuda.synchronize()
    for t in (out, gout, factor, stats, partials):
        assert (t == 7.0).all()  # no refused launch wrote anything
    # a well-formed control
    assert stat(True) == OK and step(entry) == OK
    torch.cuda.synchronize()
    assert not (out == 7.0).all() and not (gout == 7.0).all() and not (factor == 7.0).any() and not (stats == 7.0).any()


# ---- 4. rescaled guided rolling batches -----------------------------------------------------------------------------------------------
W = PD.SkrampleWrapperScheduler
MAKERS = {
    "euler": lambda sch: W(PT.Euler(), sch),
    "dpm2": lambda sch: W(PT.DPM(order=2), sch),
    "dpm2_sde": lambda sch: W(PT.DPM(order=2, stochasticity=1.0), sch),
    "adams3": lambda sch: W(PT.Adams(order=3), sch),
    "unip2": lambda sch: W(PT.UniP(order=2), sch),
}
STOCHASTIC = ("dpm2_sde",)
UNITS = {"2048": (4, 32, 16), "6144": (4, 32, 48)}
CAPACITY = 4
# (tick of admission, slot, steps, schedule, seed, guidance scale, guidance_rescale): 3, 5, 4 and 4 steps at ticks 0, 1, 1 and 3; slot 0 is
# reused once its first request has left, slot 3 stays free throughout; phi 0.7 (no fp32 value), 1.0 (psi = 0), 0.0 (never rescaled: its
# factor is never written) and a per-step schedule with zeros in it, beside a scale per request and a guidance schedule
STAGGERED = [(0, 0, 3, 0, 11, 7.3, 0.7), (1, 1, 5, 1, 12, 3.5, 1.0), (1, 2, 4, 0, 14, 2.0, 0.0), (3, 0, 4, 2, 13, (7.3, 5.1, -0.75, 2.0), (0.7, 0.0, 0.3, 0.0))]
UNRESCALED = [(*entry[:6], 0.0) for entry in STAGGERED]


def variants():
    return [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Exponential(PS.Scaled())]


def net(x, t):
    "elementwise, two halves (uncond, cond), a pure per-sample function of (latents, timestep): `t` is one float32 per sample"
    s = (t.to(torch.float32) * (1.0 / 1024.0)).to(x.dtype).view(-1, *([1] * (x.dim() - 1)))
    return x * 0.25 + (s * 0.125) * x.abs(), x * 0.125 - 0.0625 * x.abs() + s * 0.25


def per_step(value, steps):
    return list(value) if isinstance(value, tuple) else [value] * steps


def lone(kind, variant, steps, latents, seed, guidance, rescale):
    "the request alone: its own wrapper, batch 1, its own seed, step_guided with the scale and the guidance_rescale of every step"
    w = MAKERS[kind](variants()[variant])
    w.set_timesteps(steps)
    x = latents.unsqueeze(0)
    for i, t in enumerate(w.timesteps.tolist()):
        uncond, cond = net(x, torch.tensor([t], dtype=torch.float32, device=x.device))
        x = w.step_guided(uncond, cond, per_step(guidance, steps)[i], t, x, generator=[seed] if kind in STOCHASTIC else None, return_dict=False,
                          guidance_rescale=per_step(rescale, steps)[i])[0]  # fmt: skip
    return x[0].clone()


@functools.lru_cache(maxsize=None)
def yardstick(kind, dtype, unit, unrescaled=False):
    "(requests, lone results), computed once per case and shared, never written to.  requests: [(tick, slot, steps, variant, seed, guidance, rescale, latents)]"
    td, dev, g = DTYPES[dtype], torch.device("cuda:0"), torch.Generator().manual_seed(17)
    requests = [(*entry, torch.randn(UNITS[unit], generator=g).to(td).to(dev)) for entry in (UNRESCALED if unrescaled else STAGGERED)]
    refs = [lone(kind, variant, steps, latents, seed, guidance, rescale) for _, _, steps, variant, seed, guidance, rescale, latents in requests]
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs)
    return requests, refs


def serve(batch, kind, requests, tick, rescaled=True):
    "admits each request at its tick and calls `tick()` (-> finished slots) until all are done: {request number: result}"
    results, resident, at_tick = {}, {}, 0
    while len(results) < len(requests):
        for n, (at, slot, steps, variant, seed, guidance, rescale, latents) in enumerate(requests):
            if at == at_tick:
                extra = dict(guidance_rescale=list(rescale) if isinstance(rescale, tuple) else rescale) if rescaled else {}
                batch.admit(slot, latents, MAKERS[kind](variants()[variant]), steps, seed=seed if kind in STOCHASTIC else None,
                            guidance_scale=list(guidance) if isinstance(guidance, tuple) else guidance, **extra)  # fmt: skip
                resident[slot] = n
        assert batch.active
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        at_tick += 1
        assert at_tick < 32
    torch.cuda.synchronize()
    return results


def make_batch(kind, dtype, unit, dev, **options):
    example = torch.zeros((CAPACITY, *UNITS[unit]), dtype=DTYPES[dtype], device=dev)
    return RollingBatch(lambda: MAKERS[kind](variants()[0]), example, capacity=CAPACITY, guided=True, **options)


def host_tick(batch):
    return lambda: batch.step_guided(*net(batch.latents, batch.timesteps))


def check_against(results, refs, what):
    assert len(results) == len(refs)
    for n, ref in enumerate(refs):
        assert torch.equal(bits(results[n]), bits(ref)), (*what, n, int((bits(results[n]) != bits(ref)).sum()))


CASES = [(kind, dtype, unit) for kind in sorted(MAKERS) for dtype, unit in (("bf16", "2048"), ("fp16", "6144"))]
CASES += [("dpm2_sde", "bf16", "6144"), ("adams3", "fp16", "2048"), ("dpm2_sde", "fp32", "2048")]


@pytest.mark.parametrize("kind,dtype,unit", CASES)
def test_staggered_requests_equal_their_lone_rescaled_runs(kind, dtype, unit, dev):
    "4 requests of 3, 5, 4 and 4 steps, admitted at ticks 0, 1, 1 and 3, each under its own scale and its own phi: two launches a tick"
    requests, refs = yardstick(kind, dtype, unit)
    batch = make_batch(kind, dtype, unit, dev, rescaled=True)
    assert batch.rescaled and batch.roles[batch.slot] == ("o",) and tuple(batch.factor.shape) == (CAPACITY,) and batch.factor.dtype == DTYPES[dtype]
    factor_ptr, partials_ptr = batch.factor.data_ptr(), batch._partials.data_ptr()
    batch.factor[3].fill_(NAN)  # the slot that stays free: its factor is neither written nor read
    check_against(serve(batch, kind, requests, host_tick(batch)), refs, (kind, dtype, unit))
    assert not batch.active and batch._outputs == [] and batch._stamps == []  # nothing of the caller was held
    assert (batch.factor.data_ptr(), batch._partials.data_ptr()) == (factor_ptr, partials_ptr)  # allocated once, nothing per tick
    assert torch.isnan(batch.factor[3]) and torch.isfinite(batch.factor[:2].float()).all()
    assert float(batch.factor[2]) == 0.0  # the request that never rescales: its factor keeps the bytes it was built with


def test_requests_that_never_rescale_equal_their_run_in_a_guided_batch(dev):
    "phi = 0 throughout: the bits of a batch built with guided=True and without `rescaled`, and of the lone unrescaled run"
    kind, dtype, unit = "adams3", "bf16", "2048"
    requests, refs = yardstick(kind, dtype, unit, unrescaled=True)
    rescaled_refs = yardstick(kind, dtype, unit)[1]
    assert not torch.equal(bits(refs[0]), bits(rescaled_refs[0])) and torch.equal(bits(refs[2]), bits(rescaled_refs[2]))  # (phi moves a result; phi = 0 does not)
    guided = make_batch(kind, dtype, unit, dev)
    expected = serve(guided, kind, requests, host_tick(guided), rescaled=False)
    check_against(expected, refs, (kind, "guided"))
    batch = make_batch(kind, dtype, unit, dev, rescaled=True)
    batch.factor.fill_(NAN)  # never read
    check_against(serve(batch, kind, requests, host_tick(batch)), [expected[n] for n in range(len(requests))], (kind, "rescaled, phi = 0"))
    assert torch.isnan(batch.factor).all()  # never written


@pytest.mark.parametrize("kind", ["dpm2_sde", "adams3"])
def test_device_positions_and_captured_ticks_equal_the_host_published_run(kind, dev):
    dtype, unit = "bf16", "2048"
    requests, refs = yardstick(kind, dtype, unit)
    eager = make_batch(kind, dtype, unit, dev, rescaled=True, device_positions=True)

    def device_tick():
        eager.advance()
        return eager.step_guided(*net(eager.latents, eager.timesteps))

    check_against(serve(eager, kind, requests, device_tick), refs, (kind, "advance"))
    batch = make_batch(kind, dtype, unit, dev, rescaled=True, device_positions=True)
    ticks = batch.capture(net)
    assert ticks.phases == batch.keep + 2 == len(ticks.graphs) == len(ticks.outputs) == len(ticks.conds)
    factor_ptr = batch.factor.data_ptr()
    check_against(serve(batch, kind, requests, ticks.tick), refs, (kind, "captured"))
    assert ticks.ticks > ticks.phases and min(ticks.replays) >= 1 and batch.factor.data_ptr() == factor_ptr  # the same buffers in every phase
    with pytest.raises(ValueError, match="captured"):
        batch.step_guided(*net(batch.latents, batch.timesteps))


def test_admit_refusals_upload_nothing(dev):
    batch = make_batch("dpm2", "bf16", "2048", dev, rescaled=True)
    guided = make_batch("dpm2", "bf16", "2048", dev)
    x = torch.zeros(UNITS["2048"], dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="guidance_rescale must be >= 0"):
        batch.admit(0, x, MAKERS["dpm2"](PS.Scaled()), 4, guidance_scale=2.0, guidance_rescale=-0.1)
    with pytest.raises(ValueError, match="one guidance_rescale per step: 3 values for 4 steps"):
        batch.admit(0, x, MAKERS["dpm2"](PS.Scaled()), 4, guidance_scale=2.0, guidance_rescale=[0.7, 0.7, 0.7])
    with pytest.raises(ValueError, match="needs a batch built with guided=True, rescaled=True"):
        guided.admit(0, x, MAKERS["dpm2"](PS.Scaled()), 4, guidance_scale=2.0, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="rescaled=True needs guided=True"):
        RollingBatch(lambda: MAKERS["dpm2"](PS.Scaled()), torch.zeros((CAPACITY, *UNITS["2048"]), dtype=torch.bfloat16, device=dev), capacity=CAPACITY, rescaled=True)
    assert batch.free(0) and guided.free(0) and not batch.rows_dev.any() and not guided.rows_dev.any()
