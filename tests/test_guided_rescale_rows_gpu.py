"""Rescaled guidance with device-resident rows (needs an MI355X): skr_guidance_rescale_factor_indexed[_per_sample] and
skr_step_launch_guided_rescaled_indexed[_per_sample] through the C ABI, and `capture_sampling_loop(..., indexed=True, rescaled=True)` --
guidance_rescale a row value beside the guidance scale, two launches a guided step.

The yardstick of every test is code that existed before the four entries: skr_guidance_rescale_factor, skr_step_launch_guided_rescaled
and (for a row that does not rescale) skr_step_launch_guided with the row's values, the eager `step_guided(..., guidance_rescale=phi)`
loop, the `indexed=False` capture, an indexed guided capture made without `rescaled`, and the status codes of
skr_step_launch_guided_indexed[_per_sample] and skr_guidance_rescale_factor_rolling.  Every comparison is therefore bitwise; there is no
tolerance to choose.  Tables carry all-NaN junk rows around the rows a launch may read, so a wrong index shows; every index handed to a
kernel names a row of its table."""

import ctypes

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
SHAPES = [(2, 2048), (3, 6144)]  # one chunk a sample (a shift of 0, one partial), and three (the dividing branch of sample_of, stage 2's order)
NAN = float("nan")
SENTINEL = 123.0
# 1 - phi formed in double and narrowed once is NOT the fp32 subtraction for this phi (checked on the CPU below): the device must do the former
PHI_DOUBLE = 0.65


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


def padded(rows):
    "(the rows with a junk row in front of, between and behind them, the position of every row)"
    held, at = [junk_row()], []
    for row in rows:
        at.append(len(held))
        held += [row, junk_row()]
    return held, at


def test_the_named_phi_separates_the_double_subtraction_from_the_fp32_one():
    "on the CPU: (float)(1.0 - phi) != 1.0f - (float)phi for PHI_DOUBLE, and the two agree for 0.7 (so only the named phi tells them apart)"
    one = torch.tensor(1.0, dtype=torch.float32)
    assert torch.tensor(1.0 - PHI_DOUBLE, dtype=torch.float32) != one - torch.tensor(PHI_DOUBLE, dtype=torch.float32)
    assert torch.tensor(1.0 - 0.7, dtype=torch.float32) == one - torch.tensor(0.7, dtype=torch.float32)


# ---- 1. the statistics entries through the C ABI ---------------------------------------------------------------------------------------
STAT_SCALES = [7.3, -2.6, 3.3]


def stat_row(scale, phi):
    "what the statistics launch reads of a row: convert_k[0] and convert_k[1]; everything else a NaN"
    row = junk_row()
    row.convert_k[0], row.convert_k[1] = scale, phi
    return row


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


@pytest.mark.parametrize("shape", SHAPES, ids=["2x2048", "3x6144"])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_row_factor_equals_the_lone_statistics_launch(name, shape, dev):
    """both forms -- the indexed one with index_dev NULL and with a non-zero index_dev[0] plus a non-zero row_offset -- under the scales
    7.3, -2.6 and 3.3: factor, stats and partials of every sample are those of skr_guidance_rescale_factor on the sample alone (sample 1
    has mean 100 and std 0.01: the pivot); a row whose phi is 0.0 or -0.0 leaves the sentinels in factor and stats and the partials alone"""
    dtype, (B, sn) = DTYPES[name], shape
    lib, stream = _hip.load(), _hip.current_stream_ptr(dev)
    g = torch.Generator().manual_seed(300 + sn)
    u = torch.randn(shape, generator=g).to(dtype).to(dev)
    c = torch.randn(shape, generator=g).to(dtype).to(dev)
    u[1] = (100.0 + 0.01 * torch.randn(sn, generator=g)).to(dtype).to(dev)
    c[1] = (100.0 + 0.01 * torch.randn(sn, generator=g)).to(dtype).to(dev)
    want = {(s, scale): lone_factor(u[s], c[s], scale, dev, stats=True) for s in range(B) for scale in STAT_SCALES}
    assert want[(1, 7.3)][1][0] < 0.1 or dtype != torch.float32  # (the pivot sample is one: a std far below its mean)
    spans, numel, code = sn // 2048, B * sn, _hip.DTYPE_CODE[dtype]
    rows = [stat_row(scale, 0.7) for scale in STAT_SCALES] + [stat_row(5.0, 0.0), stat_row(5.0, -0.0)]
    held, at = padded(rows)
    table = upload(held, dev)

    def fresh():
        return (torch.full((B,), SENTINEL, dtype=dtype, device=dev), torch.full((2 * B,), SENTINEL, dtype=torch.float64, device=dev),
                torch.full((_hip.guidance_partials(numel, sn),), NAN, dtype=torch.float64, device=dev))  # fmt: skip

    def check(what, picked, factor, stats, partials, with_stats=True):
        "sample s read row picked[s] (a position in `rows`)"
        torch.cuda.synchronize()
        for s, k in enumerate(picked):
            part = partials[4 * spans * s : 4 * spans * (s + 1)]
            if k >= 3:  # phi = +-0: nothing written
                assert float(factor[s]) == SENTINEL and (stats[2 * s : 2 * s + 2] == SENTINEL).all() and torch.isnan(part).all(), (what, s)
                continue
            f, both, parts = want[(s, STAT_SCALES[k])]
            print(what, s, float(f[0]), both.tolist(), float(factor[s]))
            assert torch.equal(bits(factor[s : s + 1]), bits(f)), (what, s, float(factor[s]), float(f[0]))
            assert torch.equal(bits(part), bits(parts)), (what, s)  # the partials layout, unchanged
            if with_stats:
                assert torch.equal(bits(stats[2 * s : 2 * s + 2]), bits(both)), (what, s)
        if not with_stats:
            assert (stats == SENTINEL).all(), what

    for k in range(len(rows)):  # the indexed form: one row for every sample
        index = torch.tensor([at[k] - 1], dtype=torch.int32, device=dev)  # a non-zero index_dev[0] (every row sits behind a junk row) ...
        for label, tab, idx, offset in (("NULL index", upload(held[at[k] :], dev), None, 0), ("index + row_offset", table, index.data_ptr(), 1)):  # ... plus a non-zero row_offset
            factor, stats, partials = fresh()
            with_stats = k != 1  # (once without stats_dev)
            rc = lib.skr_guidance_rescale_factor_indexed(u.data_ptr(), c.data_ptr(), code, numel, sn, tab.data_ptr(), idx, offset, factor.data_ptr(),
                                                         stats.data_ptr() if with_stats else None, partials.data_ptr(), stream)  # fmt: skip
            assert rc == OK, (label, k, rc)
            check((name, shape, "indexed", label, k), [k] * B, factor, stats, partials, with_stats)
    for turn in range(5):  # the per-sample form: every sample its own row; from turn 3 on one sample's phi is 0.0 / -0.0
        picked = [(s + turn) % 3 for s in range(B)]
        if turn >= 3:
            picked[turn % B] = turn
        for offset in (0, 1):
            index = torch.tensor([at[k] - offset for k in picked], dtype=torch.int32, device=dev)
            factor, stats, partials = fresh()
            rc = lib.skr_guidance_rescale_factor_indexed_per_sample(u.data_ptr(), c.data_ptr(), code, numel, sn, table.data_ptr(), index.data_ptr(), offset, factor.data_ptr(),
                                                                    stats.data_ptr(), partials.data_ptr(), stream)  # fmt: skip
            assert rc == OK, (turn, offset, rc)
            check((name, shape, "per sample", turn, offset), picked, factor, stats, partials)


# ---- 2. the step entries through the C ABI ---------------------------------------------------------------------------------------------
COUNTS = (1, 4, 5, 8, 9, 12, 13, 16)  # every guided_kmax bucket and its edges
SCALES = [7.3, -2.6, 3.3]  # per sample; neither 7.3 nor 3.3 is an fp32 value, one scale is negative
PHIS = [PHI_DOUBLE, 0.7, 1.0]  # per sample; 0.7 is no fp32 value; 1.0: psi = 0


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


class Problem:
    "the tensors of one shape and dtype (16 operands: a launch of n takes the first n), shared by every case of a test and never written"

    def __init__(self, shape, dtype, dev, seed):
        self.shape, self.dtype, self.dev, (self.B, self.sn) = shape, dtype, dev, shape
        self.numel = self.B * self.sn
        self.g = g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(shape, generator=g).to(dtype).to(dev) for _ in range(_hip.ROW_TERMS)]
        self.cond = torch.randn(shape, generator=g).to(dtype).to(dev)
        self.seeds = torch.tensor([11, 22, 33][: self.B], dtype=torch.int64, device=dev)
        self.partials = torch.zeros(_hip.guidance_partials(self.numel, self.sn), dtype=torch.float64, device=dev)
        self.stream = _hip.current_stream_ptr(dev)
        self.lib = _hip.load()

    def pick(self):
        g = self.g
        return float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # +-[0.1, 2]

    def row(self, n, scale, phi, zeta0, stream, zero=None):
        row = _hip.StepRowC()
        for k in range(n):
            row.coef0[k] = 0.0 if k == zero else self.pick()  # (a zero coefficient still takes its fma: there is no absent operand here)
        for k in range(_hip.ROW_TERMS):
            row.coef1[k] = NAN  # not read
        row.zeta0, row.stream0 = zeta0, stream
        row.chain, row.zeta1, row.stream1 = NAN, NAN, 99  # not read
        row.convert_k[0], row.convert_k[1] = scale, phi
        row.convert_k[2] = row.convert_k[3] = NAN  # not read
        return row

    def kernarg(self, row, n, slot, noisy, store, first=0, count=None):
        """samples first .. first + count of the batch through the entries that take their scalars from the plan, with the row's values:
        skr_guidance_rescale_factor and skr_step_launch_guided_rescaled when the row's phi is not zero, skr_step_launch_guided when it is.
        (out, guided_out or None, factor or None)"""
        count = self.B if count is None else count
        numel, cut = count * self.sn, slice(first, first + count)
        plan = make_plan(n, self.dtype, self.sn, noisy)
        for k in range(n):
            plan.coef0[k] = row.coef0[k]
        plan.zeta0, plan.stream0 = row.zeta0, row.stream0
        out = torch.ones((count, self.sn), dtype=self.dtype, device=self.dev)
        guided = torch.ones((count, self.sn), dtype=self.dtype, device=self.dev) if store else None
        arr = (ctypes.c_void_p * n)(*[t[cut].data_ptr() for t in self.ops[:n]])
        guide = _hip.StepGuidanceC(self.cond[cut].data_ptr(), guided.data_ptr() if store else None, row.convert_k[0], slot, 0)
        seeds, factor = self.seeds[cut].data_ptr(), None
        if row.convert_k[1] == 0.0:
            rc = self.lib.skr_step_launch_guided(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), seeds, numel, self.stream)
        else:
            factor = torch.zeros(count, dtype=self.dtype, device=self.dev)
            partials = torch.zeros(_hip.guidance_partials(numel, self.sn), dtype=torch.float64, device=self.dev)
            rc = self.lib.skr_guidance_rescale_factor(self.ops[slot][cut].data_ptr(), self.cond[cut].data_ptr(), _hip.DTYPE_CODE[self.dtype], row.convert_k[0], numel, self.sn,
                                                      factor.data_ptr(), None, partials.data_ptr(), self.stream)  # fmt: skip
            assert rc == OK, rc
            rescale = _hip.StepRescaleC(factor.data_ptr(), row.convert_k[1], self.sn, 0)
            rc = self.lib.skr_step_launch_guided_rescaled(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(rescale), seeds, numel, self.stream)
        assert rc == OK, rc
        return out, guided, factor

    def rows_launch(self, per_sample, plan, n, slot, store, table, index, row_offset):
        "(out, guided_out or None, factor) of the statistics row launch and the rescaled row step over the batch, on factors that hold NaN"
        out = torch.full(self.shape, SENTINEL, dtype=self.dtype, device=self.dev)
        guided = torch.full(self.shape, SENTINEL, dtype=self.dtype, device=self.dev) if store else None
        factor = torch.full((self.B,), NAN, dtype=self.dtype, device=self.dev)
        self.partials.fill_(NAN)
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.ops[:n]])
        stat, step = ((self.lib.skr_guidance_rescale_factor_indexed_per_sample, self.lib.skr_step_launch_guided_rescaled_indexed_per_sample) if per_sample else
                      (self.lib.skr_guidance_rescale_factor_indexed, self.lib.skr_step_launch_guided_rescaled_indexed))  # fmt: skip
        idx = index.data_ptr() if index is not None else None
        rc = stat(self.ops[slot].data_ptr(), self.cond.data_ptr(), _hip.DTYPE_CODE[self.dtype], self.numel, self.sn, table.data_ptr(), idx, row_offset, factor.data_ptr(), None,
                  self.partials.data_ptr(), self.stream)  # fmt: skip
        assert rc == OK, rc
        guide = _hip.StepGuidanceC(self.cond.data_ptr(), guided.data_ptr() if store else None, 99.0, slot, 0)  # (guide->scale is ignored: a decoy)
        rescale = _hip.StepRescaleC(factor.data_ptr(), 0.33, self.sn, 0)  # (rescale->phi is ignored: a decoy)
        rc = step(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(rescale), self.seeds.data_ptr(), self.numel, table.data_ptr(), idx, row_offset,
                  self.stream)  # fmt: skip
        assert rc == OK, rc
        return out, guided, factor


def same(got, want, what):
    assert torch.isfinite(want.float()).all(), what
    assert torch.equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=["2x2048", "3x6144"])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_row_step_equals_the_kernarg_launches(name, shape, dev):
    """operand counts at every bucket edge, slot first / middle / last, with and without noise, guided_out given and NULL.  The indexed
    form: a rescaled row gives the bits of skr_step_launch_guided_rescaled with the row's values, a row whose phi is +-0 those of
    skr_step_launch_guided while the factor holds NaN.  The per-sample form: every sample reads a row of its own -- one of them
    unrescaled -- and equals its lone launch."""
    p = Problem(shape, DTYPES[name], dev, seed=700 + shape[1])
    B = p.B
    for n in COUNTS:
        for slot in sorted({0, n // 2, n - 1}):
            off = n % B  # the sample (and the indexed form's row) that does not rescale
            rows = [p.row(n, SCALES[s], (0.0 if n % 2 else -0.0) if s == off else PHIS[s], 0.0 if s == 1 and n == 5 else 0.3 + 0.1 * s, (3 + s) * 256, zero=n - 1 if n > 1 and s == 0 else None)
                    for s in range(B)]  # fmt: skip
            held, at = padded(rows)
            table = upload(held, dev)
            for noisy in (False, True):
                plan = decoy(make_plan(n, p.dtype, p.sn, noisy))
                stores = (True, False) if slot == n // 2 else (True,)  # once per operand count without guided_out
                for store in stores:
                    what = (name, shape, n, slot, noisy, store)
                    for k, row in enumerate(rows):  # the indexed form, every row in turn
                        want_out, want_guided, want_factor = p.kernarg(row, n, slot, noisy, store)
                        index = torch.tensor([at[k] - 1], dtype=torch.int32, device=dev)
                        for label, tab, idx, offset in (("NULL index", upload(held[at[k] :], dev), None, 0), ("index + row_offset", table, index, 1)):
                            out, guided, factor = p.rows_launch(False, plan, n, slot, store, tab, idx, offset)
                            same(out, want_out, (what, "indexed", label, k))
                            if store:
                                same(guided, want_guided, (what, "indexed", label, k, "guided_out"))
                            if k == off:
                                assert torch.isnan(factor).all(), (what, label, k)  # never written, and never read
                            else:
                                same(factor, want_factor, (what, "indexed", label, k, "factor"))
                    for offset in (0, 1):  # the per-sample form: sample s reads rows[order[s]] (with the row_offset: the last row first)
                        order = [B - 1 - s for s in range(B)] if offset else list(range(B))
                        index = torch.tensor([at[k] - offset for k in order], dtype=torch.int32, device=dev)
                        wanted = [p.kernarg(rows[order[s]], n, slot, noisy, store, first=s, count=1) for s in range(B)]
                        out, guided, factor = p.rows_launch(True, plan, n, slot, store, table, index, offset)
                        for s in range(B):
                            same(out[s], wanted[s][0][0], (what, "per sample", offset, s))
                            if store:
                                same(guided[s], wanted[s][1][0], (what, "per sample", offset, s, "guided_out"))
                            if order[s] == off:
                                assert torch.isnan(factor[s]), (what, offset, s)
                            else:
                                same(factor[s : s + 1], wanted[s][2], (what, "per sample", offset, s, "factor"))


def test_a_rescaled_row_differs_from_its_unrescaled_self_and_the_named_phi_shows_in_fp32(dev):
    """the yardsticks are not vacuous: phi = 0.7 moves the result off the unrescaled launch's; and under PHI_DOUBLE in fp32 the entry that
    is handed psi as the fp32 subtraction would give other bits (torch's own four lines with that psi differ from the launch's guided_out)"""
    p = Problem((2, 2048), torch.float32, dev, seed=77)
    n, slot = 3, 1
    rows = [p.row(n, 7.3, phi, 0.0, 256) for phi in (0.7, 0.0, PHI_DOUBLE)]
    for k in (1, 2):
        for j in range(n):
            rows[k].coef0[j] = rows[0].coef0[j]
    plan = make_plan(n, p.dtype, p.sn, False)
    outs = [p.rows_launch(False, plan, n, slot, True, upload([row], dev), None, 0) for row in rows]
    assert not torch.equal(bits(outs[0][0]), bits(outs[1][0])) and not torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    same(outs[1][1], p.kernarg(rows[1], n, slot, False, True)[1], "phi == 0 is the guided value")
    pred, r = outs[1][1], outs[2][2].reshape(2, 1)
    phi32 = torch.tensor(PHI_DOUBLE, dtype=torch.float32, device=dev)
    psi_double = torch.tensor(1.0 - PHI_DOUBLE, dtype=torch.float32, device=dev)
    psi_single = torch.tensor(1.0, dtype=torch.float32, device=dev) - phi32
    same(outs[2][1], phi32 * (pred * r) + psi_double * pred, "1 - phi in double, narrowed once")
    assert not torch.equal(bits(outs[2][1]), bits(phi32 * (pred * r) + psi_single * pred))


# ---- 3. the status tables ---------------------------------------------------------------------------------------------------------------
def test_status_tables_equal_their_yardsticks_and_nothing_is_written(dev):
    """every code of the four entries in its stated order, two-fault rows included: the step entries answer what
    skr_step_launch_guided_indexed[_per_sample] answer where the arguments are the twin's, the statistics entries what
    skr_guidance_rescale_factor_rolling answers"""
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

    twins = {False: lib.skr_step_launch_guided_indexed, True: lib.skr_step_launch_guided_indexed_per_sample}
    entries = {False: lib.skr_step_launch_guided_rescaled_indexed, True: lib.skr_step_launch_guided_rescaled_indexed_per_sample}

    def step(entry, plan=None, inputs=(a.data_ptr(), b.data_ptr()), out=out.data_ptr(), cond=cond.data_ptr(), gout=gout.data_ptr(), slot=1, reserved=0, seeds=seeds.data_ptr(),
             numel=numel, rows=table.data_ptr(), idx=index.data_ptr(), row_offset=0, no_plan=False, no_guide=False, no_inputs=False, no_rescale=False,
             factor=factor.data_ptr(), rs_numel=None, rs_reserved=0):  # fmt: skip
        plan = plan if plan is not None else plan_of()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
        head = (None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide))
        if entry in twins.values():
            return entry(*head, seeds, numel, rows, idx, row_offset, None)
        rescale = _hip.StepRescaleC(factor, 0.25, plan.sample_numel if rs_numel is None else rs_numel, rs_reserved)
        return entry(*head, None if no_rescale else ctypes.byref(rescale), seeds, numel, rows, idx, row_offset, None)

    only = dict(plan=plan_of(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a.data_ptr(),), slot=0)
    shared = [  # the twin's arguments (the statistic's sample follows the plan's)
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("no rows", dict(rows=None), NULL),
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
        ("two dtype groups", dict(plan=plan_of(n_group_a=1, dtype_b=_hip.F32)), UNSUPPORTED),
        ("acc_f64", dict(plan=plan_of(acc_f64=1)), UNSUPPORTED),
        ("a negative row_offset", dict(row_offset=-1), UNSUPPORTED),
        # two faults: the earlier check answers
        ("no rows + slot", dict(rows=None, slot=5), NULL),
        ("no seeds + slot", dict(seeds=None, slot=5), NULL),
        ("slot + negative numel", dict(slot=2, numel=-1), TERMS),
        ("negative numel + reserved", dict(numel=-1, reserved=1), SHAPE),
        ("reserved + sample size", dict(reserved=1, plan=plan_of(sample_numel=4095)), UNSUPPORTED),
        ("sample size + no cond", dict(plan=plan_of(sample_numel=4095), cond=None), SHAPE),
        ("no cond + misaligned out", dict(cond=None, out=out.data_ptr() + 4), NULL),
        ("misaligned cond + dtype", dict(cond=cond.data_ptr() + 2, plan=plan_of(out0_dtype=_hip.F16)), ALIGN),
        ("dtype + a negative row_offset", dict(plan=plan_of(out0_dtype=_hip.F16), row_offset=-1), DTYPE),
        ("acc_f64 + a negative row_offset", dict(plan=plan_of(acc_f64=1), row_offset=-1), UNSUPPORTED),
    ]
    own = [  # what the rescale descriptor adds, where skr_step_launch_guided_rescaled_rolling puts it
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
        # a workgroup lies inside one sample, with or without noise, in BOTH forms
        ("no sample size without noise", dict(plan=plan_of(noise_mode=0, sample_numel=0), rs_numel=sn), SHAPE),
        ("samples that do not divide, without noise", dict(plan=plan_of(noise_mode=0, sample_numel=numel - 2048), rs_numel=sn), SHAPE),
        ("a sample below a chunk without noise", dict(plan=plan_of(noise_mode=0, sample_numel=1024)), UNSUPPORTED),
        ("a sample below a chunk under a draw", dict(plan=plan_of(sample_numel=1024)), UNSUPPORTED),
        ("a negative row_offset + a sample below a chunk", dict(row_offset=-1, plan=plan_of(noise_mode=0, sample_numel=1024)), UNSUPPORTED),
    ]
    for per_sample in (False, True):
        for what, kwargs, want in shared:
            twin_kwargs = {k: v for k, v in kwargs.items() if k != "rs_numel"}
            assert step(entries[per_sample], **kwargs) == step(twins[per_sample], **twin_kwargs) == want, (per_sample, what)
        for what, kwargs, want in own:
            assert step(entries[per_sample], **kwargs) == want, (per_sample, what)
    assert step(entries[True], idx=None) == step(twins[True], idx=None) == NULL and step(entries[True], idx=None, slot=5) == NULL
    for key in (b"one_trip",):
        try:
            assert lib.skr_set_tuning(key, 0) == 0
            assert step(entries[False]) == step(entries[True]) == UNSUPPORTED  # there is no grid-stride form
        finally:
            lib.skr_set_tuning(key, 1)

    def stat(which, uncond=a.data_ptr(), cond=cond.data_ptr(), dtype=_hip.BF16, numel=numel, sample_numel=sn, rows=table.data_ptr(), idx=index.data_ptr(), row_offset=0,
             factor=factor.data_ptr(), partials=partials.data_ptr()):  # fmt: skip
        entry = {"rolling": lib.skr_guidance_rescale_factor_rolling, False: lib.skr_guidance_rescale_factor_indexed, True: lib.skr_guidance_rescale_factor_indexed_per_sample}[which]
        return entry(uncond, cond, dtype, numel, sample_numel, rows, idx, row_offset, factor, stats.data_ptr(), partials, None)

    for what, kwargs, want in [  # the checks of skr_guidance_rescale_factor_rolling: its codes, its order
        ("no uncond", dict(uncond=None), NULL),
        ("no cond", dict(cond=None), NULL),
        ("no factor", dict(factor=None), NULL),
        ("no partials", dict(partials=None), NULL),
        ("no rows", dict(rows=None), NULL),
        ("no partials + negative numel", dict(partials=None, numel=-1), NULL),
        ("no rows + negative numel", dict(rows=None, numel=-1), NULL),
        ("negative numel", dict(numel=-1), SHAPE),
        ("a sample of one element", dict(sample_numel=1), SHAPE),
        ("samples that do not divide", dict(sample_numel=6144), SHAPE),
        ("negative numel + misaligned uncond", dict(numel=-1, uncond=a.data_ptr() + 2), SHAPE),
        ("an empty launch", dict(numel=0), OK),
        ("an empty launch + misaligned cond + dtype", dict(numel=0, cond=cond.data_ptr() + 2, dtype=99), OK),
        ("misaligned uncond", dict(uncond=a.data_ptr() + 2), ALIGN),
        ("misaligned cond + dtype", dict(cond=cond.data_ptr() + 4, dtype=99), ALIGN),
        ("no tensor dtype", dict(dtype=99), DTYPE),
        ("dtype + a negative row_offset", dict(dtype=99, row_offset=-1), DTYPE),
        ("misaligned uncond + fp64", dict(uncond=a.data_ptr() + 2, dtype=_hip.F64), ALIGN),
        ("fp64", dict(dtype=_hip.F64), UNSUPPORTED),
        ("a sample that is no whole span", dict(numel=2 * 3072, sample_numel=3072), UNSUPPORTED),
        ("a negative row_offset", dict(row_offset=-1), UNSUPPORTED),
    ]:
        assert stat(False, **kwargs) == stat(True, **kwargs) == stat("rolling", **kwargs) == want, what
    assert stat(True, idx=None) == NULL and stat(True, idx=None, numel=-1) == NULL
    torch.cuda.synchronize()
    for t in (out, gout, factor, stats, partials):
        assert (t == 7.0).all()  # no refused launch wrote anything
    # well-formed controls: the indexed entries take a NULL index
    for per_sample, kwargs in ((False, {}), (True, {}), (False, dict(idx=None))):
        factor.fill_(7.0), out.fill_(7.0), gout.fill_(7.0)
        assert stat(per_sample, **kwargs) == OK and step(entries[per_sample], **kwargs) == OK, (per_sample, kwargs)
        torch.cuda.synchronize()
        assert not (factor == 7.0).any() and not (out == 7.0).all() and not (gout == 7.0).all()


# ---- 4. captured rescaled loops -------------------------------------------------------------------------------------------------------
LATENTS, STEPS = (2, 4, 32, 32), 6
SAMPLERS = {
    "euler": lambda: PT.Euler(),
    "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1),
    "adams3": lambda: PT.Adams(order=3),
    "unip2": lambda: PT.UniP(order=2),
}
SEEDS = [31, 32]
SCHEDULES = [lambda: PS.Karras(PS.Scaled()), lambda: PS.Scaled()]
G0, PHI0, G1, PHI1 = 7.3, 0.7, 3.3, 0.25  # the captured scale and phi, and those loaded beside another schedule


def net(x, t):  # elementwise, two outputs (uncond, cond), ignores t
    return x * 0.5 + 0.3 * x.abs(), x * 0.25 - 0.1 * x.abs()


def latents(dev, shape=LATENTS, seed=41):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).bfloat16().to(dev)


def wrapper_of(sampler, schedule=0, **fields):
    return PD.SkrampleWrapperScheduler(sampler(), SCHEDULES[schedule](), **fields)


def eager(w, x, scale, phi, seeds=SEEDS):
    "the eager twin: the same loop through step_guided, launch by launch"
    w.set_timesteps(STEPS)
    for t in w.timesteps.tolist():
        uncond, cond = net(x, t)
        x = w.step_guided(uncond, cond, scale, t, x, generator=list(seeds), return_dict=False, guidance_rescale=phi)[0]
    return x.clone()


@pytest.fixture(scope="module")
def eager_runs(dev):
    "{(sampler, schedule, scale, phi): the eager step_guided run}, computed once and shared"
    x0 = latents(dev)
    cases = [(0, G0, PHI0), (1, G1, PHI1), (0, G0, 0.0)]
    return {(name, *case): eager(wrapper_of(SAMPLERS[name], case[0]), x0, case[1], case[2]) for name in SAMPLERS for case in cases}


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_captured_rescaled_loop(name, dev, eager_runs):
    """an indexed rescaled capture equals the eager step_guided(..., guidance_rescale=phi) loop and today's indexed=False capture; slot 1
    after retarget to another schedule, scale and phi equals its eager run; retarget(guidance_rescale=0.0) equals the eager unrescaled run
    and an indexed capture made without `rescaled`"""
    x0, sampler = latents(dev), SAMPLERS[name]
    loop = capture_sampling_loop(wrapper_of(sampler), net, x0, STEPS, seeds=SEEDS, indexed=True, guidance_scale=G0, guidance_rescale=PHI0, rescaled=True)
    assert loop.rescaled and loop.guidance_rescale == PHI0 and loop.rows.rescaled and loop.rows.length == STEPS
    assert loop.rows.factor.shape == (2,) and loop.rows.factor.dtype == torch.bfloat16
    assert all(row.convert_k[0] == G0 and row.convert_k[1] == PHI0 for row in loop.rows.host[:STEPS])
    first = loop(x0)
    assert torch.equal(bits(first), bits(eager_runs[(name, 0, G0, PHI0)])), name
    frozen = capture_sampling_loop(wrapper_of(sampler), net, x0, STEPS, seeds=SEEDS, guidance_scale=G0, guidance_rescale=PHI0)
    assert frozen.rows is None and torch.equal(bits(first), bits(frozen(x0))), name
    loop.retarget(wrapper_of(sampler, 1), slot=1, guidance_scale=G1, guidance_rescale=PHI1)
    assert all(row.convert_k[0] == G1 and row.convert_k[1] == PHI1 for row in loop.rows.host[STEPS : 2 * STEPS])
    loop.retarget(wrapper_of(sampler), slot=2, guidance_rescale=0.0)
    assert all(row.convert_k[0] == G0 and row.convert_k[1] == 0.0 for row in loop.rows.host[2 * STEPS : 3 * STEPS])
    outs = [loop(x0, slot=k) for k in (0, 1, 2)]
    assert torch.equal(bits(outs[0]), bits(first)), name
    assert torch.equal(bits(outs[1]), bits(eager_runs[(name, 1, G1, PHI1)])), name
    assert torch.equal(bits(outs[2]), bits(eager_runs[(name, 0, G0, 0.0)])), name
    assert not torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])  # (the rescale is not a no-op on these inputs)
    unrescaled = capture_sampling_loop(wrapper_of(sampler), net, x0, STEPS, seeds=SEEDS, indexed=True, guidance_scale=G0)
    assert not unrescaled.rescaled and unrescaled.rows.factor is None
    assert torch.equal(bits(outs[2]), bits(unrescaled(x0))), name
    with pytest.raises(ValueError, match="captured without rescaled=True"):
        unrescaled.retarget(wrapper_of(sampler), slot=1, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="captured without rescaled=True"):
        unrescaled.retarget(wrapper_of(sampler), slot=1, guidance_rescale=0.0)


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_a_loop_captured_unrescaled_is_retargeted_to_a_phi(name, dev, eager_runs):
    "guidance_rescale=0.0, rescaled=True: the recording pass issued plain guided launches; every emitted step is two launches all the same"
    x0, sampler = latents(dev), SAMPLERS[name]
    loop = capture_sampling_loop(wrapper_of(sampler), net, x0, STEPS, seeds=SEEDS, indexed=True, guidance_scale=G0, guidance_rescale=0.0, rescaled=True)
    assert loop.rescaled and loop.rows.factor is not None and all(row.convert_k[1] == 0.0 for row in loop.rows.host[:STEPS])
    assert torch.equal(bits(loop(x0)), bits(eager_runs[(name, 0, G0, 0.0)])), name
    loop.retarget(wrapper_of(sampler), slot=0, guidance_rescale=PHI0)
    assert torch.equal(bits(loop(x0)), bits(eager_runs[(name, 0, G0, PHI0)])), name
    loop.retarget(wrapper_of(sampler, 1), slot=1, guidance_scale=G1, guidance_rescale=PHI1)
    assert torch.equal(bits(loop(x0, slot=1)), bits(eager_runs[(name, 1, G1, PHI1)])), name


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_per_sample_captured_rescaled_loop(name, dev, eager_runs):
    "per_sample=True, slots [1, 0]: every sample follows its own schedule, scale and phi, and equals its lone eager run"
    x0, sampler = latents(dev), SAMPLERS[name]
    loop = capture_sampling_loop(wrapper_of(sampler), net, x0, STEPS, seeds=SEEDS, indexed=True, per_sample=True, guidance_scale=G0, guidance_rescale=PHI0, rescaled=True)
    assert loop.per_sample and loop.rescaled
    loop.retarget(wrapper_of(sampler, 1), slot=1, guidance_scale=G1, guidance_rescale=PHI1)
    out = loop(x0, slot=[1, 0])
    settings = {0: (0, G0, PHI0), 1: (1, G1, PHI1)}
    for b, k in enumerate([1, 0]):
        schedule, scale, phi = settings[k]
        lone = eager(wrapper_of(sampler, schedule), x0[b : b + 1], scale, phi, seeds=SEEDS[b : b + 1])
        assert torch.equal(bits(out[b : b + 1]), bits(lone)), (name, b, k)
        assert torch.equal(bits(lone[0]), bits(eager_runs[(name, *settings[k])][b])), (name, b, k)  # (a sample's statistic is its own)
    assert torch.equal(bits(loop(x0, slot=0)), bits(eager_runs[(name, 0, G0, PHI0)])), name
    loop.retarget(wrapper_of(sampler), slot=2, guidance_rescale=0.0)
    mixed = loop(x0, slot=[2, 0])  # one sample unrescaled beside a rescaled one
    assert torch.equal(bits(mixed[0]), bits(eager_runs[(name, 0, G0, 0.0)][0])) and torch.equal(bits(mixed[1]), bits(eager_runs[(name, 0, G0, PHI0)][1])), name


def test_refusals_in_the_recording_pass(dev):
    "what the row kernels do not cover is refused with the reason, and no stream is capturing afterwards"
    x0 = latents(dev)

    def refused(make_loop):
        with pytest.raises(_hip.SkrampleHipError) as caught:
            make_loop()
        assert not torch.cuda.is_current_stream_capturing() and _hip.indexed is None
        text = str(caught.value)
        del caught  # (the traceback holds this frame, and the frames below it hold the loop: kept, they would be a cycle around a graph)
        return text

    unsupported = _hip.load().skr_strerror(UNSUPPORTED).decode()
    options = dict(seeds=SEEDS, indexed=True, guidance_scale=G0, guidance_rescale=PHI0, rescaled=True)
    text = refused(lambda: capture_sampling_loop(wrapper_of(lambda: PT.UniPC(order=2)), net, x0, STEPS, **options))
    assert unsupported in text and "guidance-only" in text and "UniPC" in text
    text = refused(lambda: capture_sampling_loop(wrapper_of(lambda: PT.UniPC(order=2)), net, x0, STEPS, **dict(options, guidance_rescale=0.0)))
    assert unsupported in text and "guidance-only" in text
    ragged = latents(dev, (2, 4, 24, 24))  # 2304 elements a sample: no whole chunk
    for per_sample in (False, True):
        text = refused(lambda: capture_sampling_loop(wrapper_of(SAMPLERS["euler"]), net, ragged, STEPS, per_sample=per_sample, **options))
        assert unsupported in text and "2048" in text
    whole = latents(dev, (2, 4, 24, 32))  # 6144 elements in all -- whole chunks -- in samples of 3072, which are not
    text = refused(lambda: capture_sampling_loop(wrapper_of(SAMPLERS["euler"]), net, whole, STEPS, **dict(options, guidance_rescale=0.0)))
    assert unsupported in text and "2048" in text and "rescaled" in text
    text = refused(lambda: capture_sampling_loop(wrapper_of(SAMPLERS["euler"], compute_scale=torch.float64), net, x0, STEPS, **options))
    assert unsupported in text and "float64" in text
    # a rescaled loop re-targeted with a sampler of another structure is the re-capture error, and stays as it was
    loop = capture_sampling_loop(wrapper_of(SAMPLERS["euler"]), net, x0, STEPS, **options)
    want = loop(x0)
    text = refused(lambda: loop.retarget(wrapper_of(SAMPLERS["adams3"], 1), slot=1, guidance_rescale=PHI1))
    assert "different structure" in text
    with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale must be >= 0"):
        loop.retarget(wrapper_of(SAMPLERS["euler"]), slot=1, guidance_rescale=-0.5)
    with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale is a Python number"):
        loop.retarget(wrapper_of(SAMPLERS["euler"]), slot=1, guidance_rescale="0.7")
    assert torch.equal(bits(loop(x0)), bits(want))
