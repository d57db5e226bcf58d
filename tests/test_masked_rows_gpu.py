"""Masked steps with device-resident rows (needs an MI355X): skr_step_launch_masked_indexed / _per_sample through the C ABI, and
captured in-painting loops (capture_sampling_loop(..., indexed=True[, per_sample=True]) on a wrapper with set_inpaint in force).

The yardstick of every test is code that existed before the row forms: skr_step_launch_masked with the same scalars in its plan, or the
eager set_inpaint run of the same wrapper.  Every comparison is therefore bitwise; there is no tolerance to choose."""

import ctypes
import math

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
OK, ERR_NULL, ERR_DTYPE, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 2, 5, 7
DTYPES = [torch.bfloat16, torch.float16, torch.float32]

# (latents per sample, mask per sample, one mask for the whole batch, batch): the shape vocabulary of tests/test_masked_gpu.py -- the
# smallest shapes that take each index path of the one-trip kernel
SHAPES = {
    "wraps_twice_in_a_chunk": ((4, 32, 32), (1, 32, 32), False, 3),
    "mask_spans_two_chunks": ((4, 64, 64), (1, 64, 64), False, 3),
    "wraps_mid_chunk": ((4, 96, 96), (1, 96, 96), False, 1),  # 18 chunks per sample: the dividing bps_shift form
    "batch_stride_0": ((4, 64, 64), (1, 64, 64), True, 3),
    "full_mask": ((4, 32, 32), (4, 32, 32), False, 3),
}
COUNTS = (1, 2, 5, 12, 16)


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_plan(n, dtype, sample_numel, noisy):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = _hip.DTYPE_CODE[dtype]
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel = sample_numel
    plan.noise_mode = 1 if noisy else 0
    return plan


def with_row(plan, row):
    "the plan with a row's values: what skr_step_launch_masked is given as the reference of that row"
    p = _hip.StepPlanC.from_buffer_copy(plan)
    for k in range(p.n_terms):
        p.coef0[k], p.coef1[k] = row.coef0[k], row.coef1[k]
    p.zeta0, p.stream0 = row.zeta0, row.stream0
    return p


def decoy(plan):
    "the plan an indexed launch is handed: other, non-zero scalars, which it must ignore"
    p = _hip.StepPlanC.from_buffer_copy(plan)
    for k in range(p.n_terms):
        p.coef0[k], p.coef1[k] = 9.0 + k, -7.0 - k
    p.zeta0, p.stream0 = 5.0, 77
    return p


class Problem:
    def __init__(self, name, dtype, n, dev, seed, batch=None):
        unit, munit, whole, default_batch = SHAPES[name]
        batch = default_batch if batch is None else batch
        self.shape, self.dtype, self.n, self.dev = (batch, *unit), dtype, n, dev
        self.g = g = torch.Generator().manual_seed(seed)
        self.ops = [torch.randn(self.shape, generator=g).to(dtype).to(dev) for _ in range(n)]
        mshape = (1 if whole else batch, *munit)
        self.mask = torch.rand(mshape, generator=g).to(dtype).to(dev)  # a soft mask: both forms reach every element
        self.mask_numel, self.batch_stride = lazy.mask_layout(mshape, self.shape)
        self.sample_numel = math.prod(unit)
        self.numel = math.prod(self.shape)
        self.seeds = torch.tensor([11, 22, 33][:batch], dtype=torch.int64, device=dev)
        self.arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in self.ops])
        self.desc = _hip.StepMaskC(self.mask.data_ptr(), _hip.DTYPE_CODE[dtype], 0, self.mask_numel, self.batch_stride)
        self.stream = _hip.current_stream_ptr(dev)

    def pick(self):
        g = self.g
        return float((torch.rand((), generator=g) * 1.9 + 0.1) * (1 if torch.rand((), generator=g) < 0.5 else -1))  # +-[0.1, 2]

    def row(self, kind, stream):
        "kind 0: random; 1: zeta0 = 0; 2: zeros among coef1 (every even slot, so a lone operand is absent from the known form)"
        row = _hip.StepRowC()
        for k in range(self.n):
            row.coef0[k] = self.pick()
            row.coef1[k] = 0.0 if kind == 2 and k % 2 == 0 else self.pick()
        row.zeta0, row.stream0 = (0.0 if kind == 1 else 0.3 + 0.2 * kind), stream
        row.chain, row.zeta1, row.stream1 = float("nan"), float("nan"), 99  # not read
        return row

    def kernarg(self, plan):
        out = torch.empty(self.shape, dtype=self.dtype, device=self.dev)
        rc = _hip.load().skr_step_launch_masked(ctypes.byref(plan), self.arr, out.data_ptr(), ctypes.byref(self.desc), self.seeds.data_ptr(), self.numel, self.stream)
        assert rc == OK, rc
        return out

    def indexed(self, plan, table, index, row_offset, per_sample=False):
        out = torch.empty(self.shape, dtype=self.dtype, device=self.dev)
        lib = _hip.load()
        entry = lib.skr_step_launch_masked_indexed_per_sample if per_sample else lib.skr_step_launch_masked_indexed
        rc = entry(ctypes.byref(plan), self.arr, out.data_ptr(), ctypes.byref(self.desc), self.seeds.data_ptr(), self.numel, table.data_ptr(),
                   index.data_ptr() if index is not None else None, row_offset, self.stream)  # fmt: skip
        assert rc == OK, rc
        return out


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
    return row


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_rows_equal_kernarg(name, dtype, dev):
    "row r of a table, picked by index_dev + row_offset (and by row_offset alone with index_dev = NULL) == skr_step_launch_masked with r's values"
    for n in COUNTS:
        for noisy in (False, True):
            p = Problem(name, dtype, n, dev, seed=400 + n)
            rows = [p.row(kind, 3 * 256 + kind) for kind in range(3)]
            table = upload([junk_row(), junk_row(), *rows, junk_row()], dev)
            plan = make_plan(n, dtype, p.sample_numel, noisy)
            want = [p.kernarg(with_row(plan, row)) for row in rows]
            if noisy:
                assert not torch.equal(want[0], p.kernarg(with_row(make_plan(n, dtype, p.sample_numel, False), rows[0])))  # (the draw takes part)
            for r in range(3):
                index = torch.tensor([r], dtype=torch.int32, device=dev)
                got = p.indexed(decoy(plan), table, index, 2)
                assert torch.equal(bits(got), bits(want[r])), (name, dtype, n, noisy, r, int((bits(got) != bits(want[r])).sum()))
            got = p.indexed(decoy(plan), table, None, 3)  # no index: row 0 + row_offset
            assert torch.equal(bits(got), bits(want[1])), (name, dtype, n, noisy, "NULL index")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,batch", [(name, 3) for name in SHAPES if name != "wraps_mid_chunk"] + [("wraps_mid_chunk", 2)])
def test_per_sample_rows(name, batch, dtype, dev):
    "sample b of a per-sample launch == sample b of the whole-batch indexed launch with b's row == that of the kernarg launch"
    stride = 2
    for n in COUNTS:
        for noisy in (False, True):
            p = Problem(name, dtype, n, dev, seed=500 + n, batch=batch)
            # rows 1, 3, 5 of the table (row_offset 1, entries 0 / 2 / 4); sample order [2, 0, 1]: the zeta0 = 0 row sits between noisy ones
            rows = [p.row(kind, 5 * 256 + kind) for kind in (0, 1, 2)]
            table = upload([junk_row(), rows[0], junk_row(), rows[1], junk_row(), rows[2]], dev)
            order = [2, 0, 1][:batch]
            sample_index = torch.tensor([k * stride for k in order], dtype=torch.int32, device=dev)
            plan = make_plan(n, dtype, p.sample_numel, noisy)
            got = p.indexed(decoy(plan), table, sample_index, 1, per_sample=True)
            for b, k in enumerate(order):
                whole = p.indexed(decoy(plan), table, sample_index[b : b + 1].clone(), 1)
                kernarg = p.kernarg(with_row(plan, rows[k]))
                assert torch.equal(bits(whole), bits(kernarg)), (name, dtype, n, noisy, b)
                assert torch.equal(bits(got[b]), bits(whole[b])), (name, dtype, n, noisy, b, int((bits(got[b]) != bits(whole[b])).sum()))


def test_error_codes(dev):
    "argument checks only: every call is refused before anything is launched, and the poisoned output keeps its bytes"
    p = Problem("wraps_twice_in_a_chunk", torch.bfloat16, 3, dev, seed=1)
    out = torch.full(p.shape, 7.0, dtype=p.dtype, device=dev)
    lib = _hip.load()
    table = upload([p.row(0, 1), p.row(1, 2)], dev)
    index = torch.zeros(p.shape[0], dtype=torch.int32, device=dev)
    sn, mn = p.sample_numel, p.mask_numel

    def call(per_sample, rows=table.data_ptr(), idx=index.data_ptr(), n=p.numel, arr=p.arr, mask_ptr=p.mask.data_ptr(), mask_dtype=_hip.BF16, mask_numel=mn, batch_stride=mn, row_offset=0, **fields):
        plan = make_plan(3, p.dtype, sn, False)
        for key, value in fields.items():
            setattr(plan, key, value)
        d = _hip.StepMaskC(mask_ptr, mask_dtype, 0, mask_numel, batch_stride)
        entry = lib.skr_step_launch_masked_indexed_per_sample if per_sample else lib.skr_step_launch_masked_indexed
        return entry(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(d), p.seeds.data_ptr(), n, rows, idx, row_offset, p.stream)

    for ps in (False, True):
        assert call(ps) == OK  # (the calls below differ from this one in one argument each)
        torch.cuda.synchronize()
        assert not (out == 7.0).all()
        out.fill_(7.0)
        assert call(ps, rows=None) == ERR_NULL
        assert call(ps, n=3 * 1024, sample_numel=1024) == ERR_UNSUPPORTED  # a ragged numel: no whole chunks
        assert call(ps, n=4096, sample_numel=1024) == ERR_UNSUPPORTED  # whole chunks, but a sample below a chunk
        assert call(ps, sample_numel=35 * 2048, n=3 * 35 * 2048, mask_numel=35, batch_stride=35) == ERR_UNSUPPORTED  # mask_numel % 8 != 0 (refused ahead of any access)
        assert call(ps, acc_f64=1) == ERR_UNSUPPORTED
        assert call(ps, dtype_a=_hip.F64, out0_dtype=_hip.F64, acc_f64=1, mask_dtype=_hip.F64) == ERR_UNSUPPORTED
        assert call(ps, n_group_a=2, dtype_b=_hip.F32) == ERR_UNSUPPORTED and call(ps, out0_dtype=_hip.F32) == ERR_UNSUPPORTED  # mixed dtype groups
        assert call(ps, mask_dtype=_hip.F16) == ERR_UNSUPPORTED
        assert call(ps, out1_dtype=_hip.BF16) == ERR_UNSUPPORTED
        assert call(ps, convert_to=1) == ERR_UNSUPPORTED and call(ps, convert_from=2) == ERR_UNSUPPORTED
        assert call(ps, row_offset=-1) == ERR_UNSUPPORTED
        try:
            assert lib.skr_set_tuning(b"one_trip", 0) == 0
            assert call(ps) == ERR_UNSUPPORTED  # there is no grid-stride row form
        finally:
            lib.skr_set_tuning(b"one_trip", 1)
        # the SKR_ERR_SHAPE cases of skr_step_launch_masked
        assert call(ps, mask_numel=0) == ERR_SHAPE and call(ps, mask_numel=-8) == ERR_SHAPE
        assert call(ps, mask_numel=mn - 8, batch_stride=mn - 8) == ERR_SHAPE
        assert call(ps, sample_numel=sn - 8) == ERR_SHAPE and call(ps, sample_numel=0) == ERR_SHAPE
        assert call(ps, batch_stride=8) == ERR_SHAPE and call(ps, batch_stride=-mn) == ERR_SHAPE
        assert call(ps, n=-1) == ERR_SHAPE
    assert call(True, idx=None) == ERR_NULL
    assert call(False, idx=None) == OK  # (the whole-batch entry takes a NULL index: row 0 + row_offset)
    torch.cuda.synchronize()
    out.fill_(7.0)
    assert call(False, noise_mode=1, zeta0=0.0) == OK  # the plan's zeta0 is ignored: the row decides
    torch.cuda.synchronize()
    out.fill_(7.0)
    for ps in (False, True):  # once more, all refusals in a row on a poisoned output
        for kwargs in ({"rows": None}, {"acc_f64": 1}, {"out1_dtype": _hip.BF16}, {"mask_numel": 0}, {"n": 4096, "sample_numel": 1024}):
            assert call(ps, **kwargs) != OK
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- captured in-painting loops --------------------------------------------------------------------------------------------------------
SHAPE, STEPS = (2, 4, 32, 32), 4
SAMPLERS = {
    "euler": lambda eta: PT.Euler(stochasticity=eta),
    "dpm2": lambda eta: PT.DPM(order=2, stochasticity=eta),
    "adams3": lambda eta: PT.Adams(order=3, stochasticity=eta),
    "unipc2": lambda eta: PT.UniPC(order=2, stochasticity=eta),  # two rows per step: the usual one and the masked identity form
}
LOOPS = [(name, eta) for name in SAMPLERS for eta in (0.0, 1.0)]


def net(x, t):  # elementwise, ignores t
    return x * 0.5 + 0.3 * x.abs()


def inpaint_inputs(dev, seed, shape=SHAPE):
    g = torch.Generator().manual_seed(seed)
    x, orig, nz = (torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(3))
    mask = torch.rand((shape[0], 1, *shape[2:]), generator=g) < 0.5
    mask[:, :, 0, :], mask[:, :, 1, :] = True, False
    return x, orig, nz, mask.to(dev)


def schedule_variants():
    "(schedule, begin index) of the three resident schedules: the captured one, another sigma family, a third with a begin index"
    return [(PS.Karras(PS.Scaled()), None), (PS.Scaled(), None), (PS.Karras(PS.Scaled(), rho=3.0), 1)]


def wrapper_of(name, eta, variant, inpaint):
    schedule, begin = variant
    w = PD.SkrampleWrapperScheduler(SAMPLERS[name](eta), schedule)
    if begin is not None:
        w.set_begin_index(begin)
    if inpaint is not None:
        w.set_inpaint(*inpaint)
    return w


def eager(w, x, seeds, steps=STEPS, begin=None):
    w.set_timesteps(steps)
    if begin is not None:
        w.set_begin_index(begin)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=list(seeds), return_dict=False)[0]
    return x.clone()


@pytest.mark.parametrize("name,eta", LOOPS)
def test_captured_inpainting_loop(name, eta, dev):
    "one indexed capture (one stream, no parallel branches): replay, three resident schedules, new in-paint tensors == the eager set_inpaint runs"
    seeds = [31, 32]
    x0, orig, nz, mask = inpaint_inputs(dev, 41)
    variants = schedule_variants()
    first = wrapper_of(name, eta, variants[0], (mask, orig, nz))
    loop = capture_sampling_loop(first, net, x0, STEPS, seeds=seeds, indexed=True, slots=3)
    assert loop.inpaint is not None and all(a is b for a, b in zip(loop.inpaint, first._inpaint))
    assert loop.rows.length == STEPS * (2 if name == "unipc2" else 1)
    assert torch.equal(bits(loop(x0)), bits(eager(wrapper_of(name, eta, variants[0], (mask, orig, nz)), x0, seeds)))
    for slot in (1, 2):
        loop.retarget(wrapper_of(name, eta, variants[slot], (mask, orig, nz)), slot=slot)
    outs = [loop(x0, slot=k) for k in range(3)]
    for k, variant in enumerate(variants):
        want = eager(wrapper_of(name, eta, variant, (mask, orig, nz)), x0, seeds, begin=variant[1])
        assert torch.equal(bits(outs[k]), bits(want)), (name, eta, k)
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    # another request: new in-paint tensors (a bool mask, cast as set_inpaint casts it), the resident schedule of slot 1
    _, orig2, nz2, mask2 = inpaint_inputs(dev, 43)
    got = loop(x0, slot=1, inpaint=(mask2, orig2, nz2))
    want = eager(wrapper_of(name, eta, variants[1], (mask2, orig2, nz2)), x0, seeds)
    assert torch.equal(bits(got), bits(want)) and not torch.equal(got, outs[1])
    keep = ~mask2.expand(SHAPE)
    assert torch.equal(bits(got[keep]), bits(orig2[keep]))  # after the last step the kept region is the original itself


def test_per_sample_captured_inpainting_loop(dev):
    "per_sample=True, batch 3, three resident schedules, slot = [2, 0, 1]: sample b == sample b of the whole-batch replay of its slot"
    shape, seeds, slots = (3, 4, 32, 32), [51, 52, 53], [2, 0, 1]
    x0, orig, nz, mask = inpaint_inputs(dev, 45, shape)
    variants = schedule_variants()
    for name, eta in (("dpm2", 1.0), ("unipc2", 1.0)):
        loop = capture_sampling_loop(wrapper_of(name, eta, variants[0], (mask, orig, nz)), net, x0, STEPS, seeds=seeds, indexed=True, slots=3, per_sample=True)
        assert loop.per_sample
        for slot in (1, 2):
            loop.retarget(wrapper_of(name, eta, variants[slot], (mask, orig, nz)), slot=slot)
        out = loop(x0, slot=slots)
        for b, k in enumerate(slots):
            uniform = loop(x0, slot=k)
            assert torch.equal(bits(out[b]), bits(uniform[b])), (name, b, k)
            want = eager(wrapper_of(name, eta, variants[k], (mask, orig, nz)), x0, seeds, begin=variants[k][1])
            assert torch.equal(bits(uniform), bits(want)), (name, k)


def test_refusals_before_capture(dev):
    "what the row kernel does not cover is refused in the recording pass, while no stream is capturing"
    variants = schedule_variants()

    def refused(make_loop):
        with pytest.raises(_hip.SkrampleHipError) as caught:
            make_loop()
        assert not torch.cuda.is_current_stream_capturing() and _hip.indexed is None
        return str(caught.value)

    small = (2, 4, 16, 16)  # a sample below a chunk
    x0, orig, nz, mask = inpaint_inputs(dev, 47, small)
    text = refused(lambda: capture_sampling_loop(wrapper_of("euler", 0.0, variants[0], (mask, orig, nz)), net, x0, STEPS, indexed=True))
    assert _hip.load().skr_strerror(ERR_UNSUPPORTED).decode() in text and "2048" in text

    x0, orig, nz, mask = inpaint_inputs(dev, 49)
    wide = PD.SkrampleWrapperScheduler(PT.Euler(), variants[0][0], compute_scale=torch.float64)
    wide.set_inpaint(mask, orig, nz)
    text = refused(lambda: capture_sampling_loop(wide, net, x0, STEPS, indexed=True))
    assert _hip.load().skr_strerror(ERR_UNSUPPORTED).decode() in text

    loop = capture_sampling_loop(wrapper_of("dpm2", 0.0, variants[0], (mask, orig, nz)), net, x0, STEPS, indexed=True)
    text = refused(lambda: loop.retarget(wrapper_of("dpm2", 0.0, variants[1], None), slot=1))  # no in-painting set against a masked capture
    assert "different structure" in text
    assert torch.equal(bits(loop(x0)), bits(eager(wrapper_of("dpm2", 0.0, variants[0], (mask, orig, nz)), x0, [0, 0])))  # the loop is as it was

    plain = capture_sampling_loop(wrapper_of("dpm2", 0.0, variants[0], None), net, x0, STEPS, indexed=True)
    assert plain.inpaint is None
    with pytest.raises(ValueError):
        plain(x0, inpaint=(mask, orig, nz))
    text = refused(lambda: plain.retarget(wrapper_of("dpm2", 0.0, variants[1], (mask, orig, nz)), slot=1))  # and the reverse
    assert "different structure" in text
