"""Guided steps with device-resident rows (needs an MI355X): skr_step_launch_guided_indexed / _per_sample through the C ABI, and captured
classifier-free-guidance loops (capture_sampling_loop(..., guidance_scale=g[, indexed=True[, per_sample=True]])).

The yardstick of every test is code that existed before the row forms: skr_step_launch_guided with the row's values in its plan and in
guide->scale, or the eager step_guided run of a twin wrapper.  Every comparison is therefore bitwise; there is no tolerance to choose.
The scales are 7.3 and 3.3, neither of which is an fp32 value: a row's double must be narrowed once, as the host narrows guide->scale."""

import ctypes
import gc
import math

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
# one chunk per sample (a shift of 0), and three chunks per sample: not a power of two, the dividing branch of sample_of
SHAPES = {"one_chunk": (2, 2048), "three_chunks": (3, 6144)}


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def no_graph_outlives_its_test():
    """A captured loop that a dead reference cycle holds is destroyed whenever the collector next runs, and inside a later capture that
    ends the process (graphs._no_collection says why).  The tests below keep no caught exception beyond the block that caught it, and
    what is left is collected here, while no stream captures."""
    yield
    gc.collect()


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def slots_of(n):
    return sorted({0, n // 2, n - 1})


def make_plan(n, dtype, sample_numel, noisy):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = _hip.DTYPE_CODE[dtype]
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel = sample_numel
    plan.noise_mode = 1 if noisy else 0
    return plan


def with_row(plan, row):
    "the plan with a row's values: what skr_step_launch_guided is given as the reference of that row (with the row's scale in the guide)"
    p = _hip.StepPlanC.from_buffer_copy(plan)
    for k in range(p.n_terms):
        p.coef0[k] = row.coef0[k]
    p.zeta0, p.stream0 = row.zeta0, row.stream0
    return p


def decoy(plan):
    "the plan a row launch is handed: other, non-zero scalars, which it must ignore"
    p = _hip.StepPlanC.from_buffer_copy(plan)
    for k in range(p.n_terms):
        p.coef0[k], p.coef1[k] = 9.0 + k, -7.0 - k
    p.zeta0, p.stream0 = 5.0, 77
    return p


def upload(rows, dev):
    table = torch.zeros(len(rows) * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
    _hip.upload_rows(table, 0, rows)
    return table


def junk_row():
    "a row no launch of these tests may read: every double a NaN"
    row = _hip.StepRowC()
    for k in range(_hip.ROW_TERMS):
        row.coef0[k] = row.coef1[k] = float("nan")
    row.zeta0 = row.chain = row.zeta1 = float("nan")
    for k in range(4):
        row.convert_k[k] = float("nan")
    return row


class Problem:
    "the tensors of one shape and dtype (16 operands: a launch of n takes the first n), shared by every case of a test"

    def __init__(self, shape, dtype, dev, seed):
        self.shape, self.dtype, self.dev = shape, dtype, dev
        self.g = g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(shape, generator=g).to(dtype).to(dev) for _ in range(_hip.ROW_TERMS)]
        self.cond = torch.randn(shape, generator=g).to(dtype).to(dev)
        self.sample_numel, self.numel = math.prod(shape[1:]), math.prod(shape)
        self.seeds = torch.tensor([11, 22, 33][: shape[0]], dtype=torch.int64, device=dev)
        self.stream = _hip.current_stream_ptr(dev)

    def pick(self):
        g = self.g
        return float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # +-[0.1, 2]

    def row(self, n, scale, zeta0, stream):
        row = _hip.StepRowC()
        for k in range(n):
            row.coef0[k] = self.pick()
        for k in range(_hip.ROW_TERMS):
            row.coef1[k] = float("nan")  # not read
        row.zeta0, row.stream0 = zeta0, stream
        row.chain, row.zeta1, row.stream1 = float("nan"), float("nan"), 99  # not read
        row.convert_k[0] = scale
        row.convert_k[1] = row.convert_k[2] = row.convert_k[3] = float("nan")  # not read
        return row

    def launch(self, entry, plan, n, slot, scale, store, *tail):
        "(out, guided_out or None) of one launch of `entry`, on outputs poisoned with ones"
        out = torch.ones(self.shape, dtype=self.dtype, device=self.dev)
        guided = torch.ones(self.shape, dtype=self.dtype, device=self.dev) if store else None
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.ops[:n]])
        guide = _hip.StepGuidanceC(self.cond.data_ptr(), guided.data_ptr() if store else None, scale, slot, 0)
        rc = entry(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), self.seeds.data_ptr(), self.numel, *tail, self.stream)
        assert rc == OK, rc
        return out, guided

    def kernarg(self, plan, n, slot, scale, store):
        return self.launch(_hip.load().skr_step_launch_guided, plan, n, slot, scale, store)

    def indexed(self, plan, n, slot, store, table, index, row_offset, per_sample=False):
        lib = _hip.load()
        entry = lib.skr_step_launch_guided_indexed_per_sample if per_sample else lib.skr_step_launch_guided_indexed
        # (guide->scale is ignored by a row launch: a decoy)
        return self.launch(entry, plan, n, slot, 99.0, store, table.data_ptr(), index.data_ptr() if index is not None else None, row_offset)


def same(got, want):
    "both outputs of two launches equal in every bit"
    return all((g is None and w is None) or torch.equal(bits(g), bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_rows_equal_kernarg(name, shape, dev):
    """row r of a table, picked by index_dev[0] + row_offset (both non-zero, among NaN rows; and by row_offset alone with index_dev =
    NULL) == skr_step_launch_guided with r's values: every operand count, slot first / middle / last, with and without noise, with
    and without guided_out.  Row A draws with scale 7.3, row B has zeta0 = 0 and scale 3.3: under a drawing plan it equals the
    launch without noise."""
    p = Problem(SHAPES[shape], DTYPES[name], dev, seed=600)
    indices = [torch.tensor([1 + r], dtype=torch.int32, device=dev) for r in range(2)]
    for n in range(1, _hip.ROW_TERMS + 1):
        rows = [p.row(n, 7.3, 0.45, 3 * 256), p.row(n, 3.3, 0.0, 3 * 256 + 1)]
        table = upload([junk_row(), junk_row(), rows[0], rows[1], junk_row()], dev)
        for slot in slots_of(n):
            for noisy, store in ((False, False), (False, True), (True, False), (True, True)):
                plan = make_plan(n, p.dtype, p.sample_numel, noisy)
                what = (name, shape, n, slot, noisy, store)
                want = [p.kernarg(with_row(plan, row), n, slot, row.convert_k[0], store) for row in rows]
                quiet = [p.kernarg(with_row(make_plan(n, p.dtype, p.sample_numel, False), row), n, slot, row.convert_k[0], store) for row in rows]
                assert same(want[0], quiet[0]) != noisy, what  # (the draw takes part exactly when the plan and the row say so)
                assert same(want[1], quiet[1]) and not same(want[0], want[1]), what
                for r in range(2):
                    got = p.indexed(decoy(plan), n, slot, store, table, indices[r], 1)
                    assert same(got, want[r]), (what, r, int((bits(got[0]) != bits(want[r][0])).sum()))
                assert same(p.indexed(decoy(plan), n, slot, store, table, None, 3), want[1]), (what, "NULL index")


@pytest.mark.parametrize("shape", [(3, 2048), (3, 6144)], ids=["one_chunk", "three_chunks"])
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_per_sample_rows(name, shape, dev):
    """three samples follow three different rows (other coefficients, other scale, one with zeta0 = 0): sample b of the per-sample launch
    == sample b of the whole-batch indexed launch with b's row == that of the kernarg launch"""
    p = Problem(shape, DTYPES[name], dev, seed=700)
    for n in (1, 2, 3, 4, 5, 8, 9, 12, 13, 16):
        # rows 1, 3, 5 of the table (row_offset 1, entries 0 / 2 / 4); sample order [2, 0, 1]: the zeta0 = 0 row sits between drawing ones
        rows = [p.row(n, 7.3, 0.45, 5 * 256), p.row(n, 3.3, 0.0, 5 * 256 + 1), p.row(n, 1.7, 0.8, 5 * 256 + 2)]
        table = upload([junk_row(), rows[0], junk_row(), rows[1], junk_row(), rows[2]], dev)
        order = [2, 0, 1]
        sample_index = torch.tensor([2 * k for k in order], dtype=torch.int32, device=dev)
        for slot in slots_of(n):
            for noisy in (False, True):
                store = (slot + noisy) % 2 == 0
                plan = make_plan(n, p.dtype, p.sample_numel, noisy)
                got = p.indexed(decoy(plan), n, slot, store, table, sample_index, 1, per_sample=True)
                for b, k in enumerate(order):
                    whole = p.indexed(decoy(plan), n, slot, store, table, sample_index[b : b + 1].clone(), 1)
                    assert same(whole, p.kernarg(with_row(plan, rows[k]), n, slot, rows[k].convert_k[0], store)), (name, shape, n, slot, noisy, b)
                    assert same([t[b] if t is not None else None for t in got], [t[b] if t is not None else None for t in whole]), (name, shape, n, slot, noisy, b)
                if not noisy and n > 1:  # (the three samples did follow three rows)
                    assert not torch.equal(bits(got[0][0]), bits(p.indexed(decoy(plan), n, slot, store, table, None, 1)[0][0]))


def test_status_table_in_order_and_nothing_written(dev):
    """skr_step_launch_guided's checks in its order and with its codes, the rows' on top of them, two-fault rows for adjacent checks,
    every SKR_ERR_UNSUPPORTED case of the header, and the poisoned outputs keep their bytes"""
    lib = _hip.load()
    numel, sn = 8192, 4096
    g = torch.Generator().manual_seed(800)
    a, b, cond = (torch.randn((2, sn), generator=g).bfloat16().to(dev) for _ in range(3))
    wide = [torch.randn((2, sn), generator=g).to(dev) for _ in range(5)]  # fp32 tensors: operands, cond and outputs of the "tile" case
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

    def call(per_sample, plan=None, inputs=(a.data_ptr(), b.data_ptr()), out=out.data_ptr(), cond=cond.data_ptr(), gout=gout.data_ptr(), slot=1, reserved=0,
             seeds=seeds.data_ptr(), numel=numel, rows=table.data_ptr(), idx=index.data_ptr(), row_offset=0, no_plan=False, no_guide=False, no_inputs=False):  # fmt: skip
        plan = plan if plan is not None else plan_of()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, 7.5, slot, reserved)
        entry = lib.skr_step_launch_guided_indexed_per_sample if per_sample else lib.skr_step_launch_guided_indexed
        return entry(None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide), seeds, numel, rows, idx, row_offset, None)

    only = dict(plan=plan_of(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a.data_ptr(),), slot=0)
    fp32 = dict(inputs=(wide[0].data_ptr(), wide[1].data_ptr()), cond=wide[2].data_ptr(), out=out32.data_ptr(), gout=gout32.data_ptr())
    table_of_cases = [
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("no rows", dict(rows=None), NULL),
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
        ("an fp64 group for the slot without acc_f64", dict(plan=plan_of(n_group_a=1, dtype_b=_hip.F64)), DTYPE),
        ("an out dtype outside the groups", dict(plan=plan_of(out0_dtype=_hip.F16)), DTYPE),
        # what the one-trip kernel does not cover: there is no grid-stride row form
        ("a ragged size", dict(numel=numel - 8, plan=plan_of(noise_mode=0)), UNSUPPORTED),
        ("a sample below a chunk under a draw", dict(numel=4096, plan=plan_of(sample_numel=1024)), UNSUPPORTED),
        ("two dtype groups", dict(plan=plan_of(n_group_a=1, dtype_b=_hip.F32)), UNSUPPORTED),
        ("an fp32 output of bf16 operands", dict(plan=plan_of(out0_dtype=_hip.F32)), UNSUPPORTED),
        ("fp64", dict(plan=plan_of(dtype_a=_hip.F64, out0_dtype=_hip.F64, acc_f64=1)), UNSUPPORTED),
        ("acc_f64", dict(plan=plan_of(acc_f64=1)), UNSUPPORTED),
        ("the guidance-only form", dict(only, out=None), UNSUPPORTED),
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
    for per_sample in (False, True):
        for what, kwargs, want in table_of_cases:
            assert call(per_sample, **kwargs) == want, (per_sample, what)
        for key, tensors in ((b"one_trip", {}), (b"tile", fp32)):
            try:
                assert lib.skr_set_tuning(key, 0) == 0
                fields = dict(tensors, plan=plan_of(dtype_a=_hip.F32, out0_dtype=_hip.F32)) if tensors else {}
                assert call(per_sample, **fields) == UNSUPPORTED, (per_sample, key)
            finally:
                lib.skr_set_tuning(key, 1)
    # the per-sample entry: a workgroup lies inside one sample, with or without noise
    assert call(True, idx=None) == NULL and call(True, idx=None, slot=5) == NULL
    for noise_mode in (0, 1):
        assert call(True, plan=plan_of(noise_mode=noise_mode, sample_numel=0)) == SHAPE
        assert call(True, plan=plan_of(noise_mode=noise_mode, sample_numel=numel - 2048)) == SHAPE
        assert call(True, plan=plan_of(noise_mode=noise_mode, sample_numel=1024)) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (out, gout, out32, gout32):
        assert (t == 7.0).all()  # no refused launch wrote anything
    # well-formed controls: the whole-batch entry takes a NULL index, and the plan's zeta0 is ignored (the row decides)
    for per_sample, kwargs in ((False, {}), (True, {}), (False, dict(idx=None)), (False, dict(plan=plan_of(zeta0=0.0))), (False, dict(plan=plan_of(noise_mode=0, sample_numel=0)))):
        out.fill_(7.0), gout.fill_(7.0)
        assert call(per_sample, **kwargs) == OK, (per_sample, kwargs)
        torch.cuda.synchronize()
        assert not (out == 7.0).all() and not (gout == 7.0).all()


# ---- captured guided loops -----------------------------------------------------------------------------------------------------------
LATENTS, STEPS = (2, 4, 32, 32), 6
ONE_LAUNCH = {
    "euler": lambda: PT.Euler(),
    "dpm2": lambda: PT.DPM(order=2),
    "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1),
    "adams3": lambda: PT.Adams(order=3),
    "unip2": lambda: PT.UniP(order=2),
}
SEEDS = [31, 32]
# (schedule, guidance scale) of the resident slots: the captured one, and another sigma family with another scale
VARIANTS = [(lambda: PS.Karras(PS.Scaled()), 7.3), (lambda: PS.Scaled(), 3.3)]


def net(x, t):  # elementwise, two outputs (uncond, cond), ignores t
    return x * 0.5 + 0.3 * x.abs(), x * 0.25 - 0.1 * x.abs()


def plain_net(x, t):
    return net(x, t)[0]


def latents(dev, seed=41):
    return torch.randn(LATENTS, generator=torch.Generator().manual_seed(seed)).bfloat16().to(dev)


def wrapper_of(sampler, variant=0, **fields):
    return PD.SkrampleWrapperScheduler(sampler(), VARIANTS[variant][0](), **fields)


def eager(w, x, scale):
    "the eager twin: the same loop through step_guided, launch by launch"
    w.set_timesteps(STEPS)
    for t in w.timesteps.tolist():
        uncond, cond = net(x, t)
        x = w.step_guided(uncond, cond, scale, t, x, generator=list(SEEDS), return_dict=False)[0]
    return x.clone()


@pytest.fixture(scope="module")
def eager_runs(dev):
    "{(sampler, variant): the eager step_guided run}, computed once and shared"
    x0 = latents(dev)
    return {(name, v): eager(wrapper_of(ONE_LAUNCH[name], v), x0, VARIANTS[v][1]) for name in ONE_LAUNCH for v in range(len(VARIANTS))}


@pytest.mark.parametrize("name", sorted(ONE_LAUNCH))
def test_captured_guided_loop(name, dev, eager_runs):
    "an indexed guided capture: the replay, and slot 1 after retarget to another schedule AND scale, equal the eager step_guided runs"
    x0 = latents(dev)
    loop = capture_sampling_loop(wrapper_of(ONE_LAUNCH[name]), net, x0, STEPS, seeds=SEEDS, indexed=True, guidance_scale=VARIANTS[0][1])
    assert loop.guidance_scale == 7.3 and loop.rows.guided and loop.rows.length == STEPS
    assert all(row.convert_k[0] == 7.3 for row in loop.rows.host[:STEPS])
    assert torch.equal(bits(loop(x0)), bits(eager_runs[(name, 0)])), name
    loop.retarget(wrapper_of(ONE_LAUNCH[name], 1), slot=1, guidance_scale=VARIANTS[1][1])
    assert all(row.convert_k[0] == 3.3 for row in loop.rows.host[STEPS : 2 * STEPS])
    outs = [loop(x0, slot=k) for k in (0, 1)]
    for k in (0, 1):
        assert torch.equal(bits(outs[k]), bits(eager_runs[(name, k)])), (name, k)
    assert not torch.equal(outs[0], outs[1])
    # the default of retarget is the captured scale: the second schedule under 7.3 is a third result
    loop.retarget(wrapper_of(ONE_LAUNCH[name], 1), slot=2)
    assert torch.equal(bits(loop(x0, slot=2)), bits(eager(wrapper_of(ONE_LAUNCH[name], 1), x0, 7.3))), name


@pytest.mark.parametrize("name", sorted(ONE_LAUNCH))
def test_per_sample_captured_guided_loop(name, dev, eager_runs):
    "per_sample=True, slot = [1, 0]: each sample has the bits of its whole-batch slot, which are the eager run's"
    x0 = latents(dev)
    loop = capture_sampling_loop(wrapper_of(ONE_LAUNCH[name]), net, x0, STEPS, seeds=SEEDS, indexed=True, per_sample=True, guidance_scale=VARIANTS[0][1])
    assert loop.per_sample
    loop.retarget(wrapper_of(ONE_LAUNCH[name], 1), slot=1, guidance_scale=VARIANTS[1][1])
    out = loop(x0, slot=[1, 0])
    for b, k in enumerate([1, 0]):
        uniform = loop(x0, slot=k)
        assert torch.equal(bits(uniform), bits(eager_runs[(name, k)])), (name, k)
        assert torch.equal(bits(out[b]), bits(uniform[b])), (name, b, k)
    assert not torch.equal(out[0], loop(x0, slot=0)[0])


def test_unipc_is_refused_with_rows_and_captured_without(dev):
    "the guidance of a two-output sampler is a launch of its own, which has no row form; a plain capture freezes the scale and serves it"
    x0 = latents(dev)
    unipc = lambda: PT.UniPC(order=2)  # noqa: E731
    with pytest.raises(_hip.SkrampleHipError) as caught:
        capture_sampling_loop(wrapper_of(unipc), net, x0, STEPS, seeds=SEEDS, indexed=True, guidance_scale=7.3)
    text = str(caught.value)
    del caught  # (a caught exception kept in its own frame is a reference cycle)
    assert not torch.cuda.is_current_stream_capturing() and _hip.indexed is None
    assert _hip.load().skr_strerror(UNSUPPORTED).decode() in text and "guidance-only" in text and "UniPC" in text
    loop = capture_sampling_loop(wrapper_of(unipc), net, x0, STEPS, seeds=SEEDS, guidance_scale=7.3)
    assert loop.rows is None and loop.guidance_scale == 7.3
    assert torch.equal(bits(loop(x0)), bits(eager(wrapper_of(unipc), x0, 7.3)))
    x1 = latents(dev, 43)
    assert torch.equal(bits(loop(x1)), bits(eager(wrapper_of(unipc), x1, 7.3)))  # (a replay on other latents)


def test_refusals_before_capture_and_on_unguided_loops(dev):
    "what the row kernel does not cover is refused in the recording pass, while no stream is capturing; an unguided loop takes no scale"
    x0 = latents(dev)

    def refused(make_loop):
        with pytest.raises(_hip.SkrampleHipError) as caught:
            make_loop()
        assert not torch.cuda.is_current_stream_capturing() and _hip.indexed is None
        text = str(caught.value)
        del caught  # (the traceback holds this frame, and the frames below it hold the loop: kept, they would be a cycle around a graph)
        return text

    unsupported = _hip.load().skr_strerror(UNSUPPORTED).decode()
    dpm2 = ONE_LAUNCH["dpm2"]
    text = refused(lambda: capture_sampling_loop(wrapper_of(dpm2, compute_scale=torch.float64), net, x0, STEPS, indexed=True, guidance_scale=7.3))
    assert unsupported in text and "float64" in text
    text = refused(lambda: capture_sampling_loop(wrapper_of(dpm2, compute_scale=None), net, x0, STEPS, indexed=True, guidance_scale=7.3))
    assert unsupported in text and "guidance-only" in text
    g = torch.Generator().manual_seed(5)
    orig, nz = (torch.randn(LATENTS, generator=g).bfloat16().to(dev) for _ in range(2))
    masked = wrapper_of(dpm2)
    masked.set_inpaint((torch.rand((2, 1, 32, 32), generator=g) < 0.5).to(dev), orig, nz)
    text = refused(lambda: capture_sampling_loop(masked, net, x0, STEPS, indexed=True, guidance_scale=7.3))
    assert unsupported in text and "set_inpaint" in text
    small = x0[:, :, :16, :16].contiguous()  # a sample below a chunk: no workgroup of a per-sample launch lies inside one
    text = refused(lambda: capture_sampling_loop(wrapper_of(dpm2), net, small, STEPS, indexed=True, per_sample=True, guidance_scale=7.3))
    assert unsupported in text and "2048" in text
    # a loop captured without guidance: its hook refuses a guided launch, and retarget takes no scale
    plain = capture_sampling_loop(wrapper_of(dpm2), plain_net, x0, STEPS, indexed=True)
    assert plain.guidance_scale is None and not plain.rows.guided
    with pytest.raises(ValueError, match="captured without guidance"):
        plain.retarget(wrapper_of(dpm2, 1), slot=1, guidance_scale=3.3)
    before = plain(x0)
    plain.retarget(wrapper_of(dpm2, 1), slot=1)
    assert torch.equal(bits(plain(x0, slot=0)), bits(before)) and not torch.equal(plain(x0, slot=1), before)
    # a guided loop re-targeted with a sampler of another structure is the re-capture error, and stays as it was
    guided = capture_sampling_loop(wrapper_of(dpm2), net, x0, STEPS, seeds=SEEDS, indexed=True, guidance_scale=7.3)
    want = guided(x0)
    text = refused(lambda: guided.retarget(wrapper_of(ONE_LAUNCH["adams3"], 1), slot=1, guidance_scale=3.3))
    assert "different structure" in text
    assert torch.equal(bits(guided(x0)), bits(want))
