"""The status every elementwise entry point answers a malformed raw call with, and the order of its checks: what tests/test_masked_gpu.py
pins for skr_step_launch_masked, for skr_step_launch, the three table forms, skr_program_create, skr_step_backward_launch, skr_error_mean,
skr_power_blend, skr_power_blend_backward, skr_noise_random and the three Pyramid generators (skr_noise_pyramid, skr_noise_pyramid_any,
skr_noise_pyramid_nd; their units and the one exception to "before anything is launched" stand with their tables at the end).

One 2048-element chunk per operand, three operands, bf16 (and one fp32 case per entry point).  Every table row is refused before anything is
launched -- the outputs stay zero --; the one well-formed control per entry point follows its table.  A row that is wrong in two ways pins
the order of two adjacent checks: it must answer with the status of the earlier one."""

import ctypes

import pytest
import torch

from skrample_amd import _hip

pytestmark = pytest.mark.gpu
OK, ERR_NULL, ERR_DTYPE, ERR_TERMS, ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5, 7
N, NUMEL = 3, 2048
BAD = 9  # no skr_dtype


class Box:
    "operands, outputs, seeds and a one-row table of one dtype on the device"

    def __init__(self, dtype, dev):
        g = torch.Generator().manual_seed(5)
        self.dtype, self.code, self.dev = dtype, _hip.DTYPE_CODE[dtype], dev
        self.ops = [torch.randn(NUMEL, generator=g).to(dtype).to(dev) for _ in range(N)]
        self.out0, self.out1 = (torch.zeros(NUMEL, dtype=dtype, device=dev) for _ in range(2))
        self.wide = torch.zeros(NUMEL, dtype=torch.float32, device=dev)
        self.grads = [torch.zeros(NUMEL, dtype=dtype, device=dev) for _ in range(N)]
        self.seeds = torch.tensor([11], dtype=torch.int64, device=dev)
        self.index = torch.zeros(1, dtype=torch.int32, device=dev)
        row = _hip.StepRowC()
        for k in range(N):
            row.coef0[k] = 0.5 + k
        self.rows = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
        _hip.upload_rows(self.rows, 0, [row])
        self.scalar = torch.zeros(1, dtype=torch.float64, device=dev)
        self.partials = torch.zeros(1024, dtype=torch.float64, device=dev)
        self.stream = _hip.current_stream_ptr(dev)

    def ptrs(self, tensors, **replace):
        "the pointer array of `tensors`; replace={index: pointer or None}"
        arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        for k, v in replace.items():
            arr[int(k)] = v
        return arr

    def untouched(self):
        torch.cuda.synchronize()
        return not any(t.any() for t in (self.out0, self.out1, self.wide, self.scalar, *self.grads))


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bf(dev):
    return Box(torch.bfloat16, dev)


@pytest.fixture(scope="module")
def f32(dev):
    return Box(torch.float32, dev)


def step_plan(box, **fields):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = N
    plan.dtype_a = plan.out0_dtype = box.code
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel = NUMEL
    for k in range(N):
        plan.coef0[k] = 0.5 + k
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


NOISY = dict(noise_mode=1, zeta0=0.5)
# the checks of validate_plan, in their order; shared by the launches and skr_program_create.  (label, plan fields, numel, status)
PLAN_ROWS = [
    ("n_terms above the maximum", dict(n_terms=81, n_group_a=81), NUMEL, ERR_TERMS),
    ("n_terms negative", dict(n_terms=-1, n_group_a=-1), NUMEL, ERR_TERMS),
    ("group a beyond the terms", dict(n_group_a=4), NUMEL, ERR_TERMS),
    ("group a negative", dict(n_group_a=-1), NUMEL, ERR_TERMS),
    ("terms before numel", dict(n_terms=81, n_group_a=81), -1, ERR_TERMS),
    ("numel negative", dict(), -1, ERR_SHAPE),
    ("numel before the missing outputs", dict(out0_dtype=_hip.NONE), -1, ERR_SHAPE),
    ("no output at all", dict(out0_dtype=_hip.NONE), NUMEL, ERR_NULL),
    ("missing outputs before the noise mode", dict(out0_dtype=_hip.NONE, noise_mode=2), NUMEL, ERR_NULL),
    ("noise mode 2", dict(noise_mode=2), NUMEL, ERR_UNSUPPORTED),
    ("noise mode negative", dict(noise_mode=-1), NUMEL, ERR_UNSUPPORTED),
    ("conversion kind 4", dict(convert_to=4, out1_dtype=_hip.BF16), NUMEL, ERR_UNSUPPORTED),
    ("conversion kind negative", dict(convert_from=-1, out1_dtype=_hip.BF16), NUMEL, ERR_UNSUPPORTED),
    ("conversion range before its operands", dict(convert_to=4), NUMEL, ERR_UNSUPPORTED),
    ("conversion without out1", dict(convert_to=1), NUMEL, ERR_TERMS),
    ("conversion with one operand in group a", dict(convert_from=2, n_group_a=1, out1_dtype=_hip.BF16), NUMEL, ERR_TERMS),
    ("conversion operands before the sample size", dict(convert_to=1, sample_numel=0, **NOISY), NUMEL, ERR_TERMS),
    ("a draw without a sample size", dict(sample_numel=0, **NOISY), NUMEL, ERR_SHAPE),
    ("a draw over samples that do not divide numel", dict(sample_numel=1000, **NOISY), NUMEL, ERR_SHAPE),
    ("a draw over samples of no multiple of 8", dict(sample_numel=4, **NOISY), NUMEL, ERR_UNSUPPORTED),
    ("a second-output draw over samples of no multiple of 8", dict(sample_numel=4, noise_mode=1, zeta1=0.5, out1_dtype=_hip.BF16), NUMEL, ERR_UNSUPPORTED),
]


def launch_rows(b):
    "(label, plan fields, call arguments, status) of skr_step_launch and, with a table, of the table forms: step_launch_impl's own checks around PLAN_ROWS"
    mis = b.ops[1].data_ptr() + 2
    rows = [
        ("no plan", None, dict(), ERR_NULL),
        ("a draw without seeds", NOISY, dict(), ERR_NULL),
        ("missing seeds before the plan's checks", dict(n_terms=81, n_group_a=81, **NOISY), dict(), ERR_NULL),
        ("missing seeds before the sample size", dict(sample_numel=0, **NOISY), dict(), ERR_NULL),
    ]
    rows += [(label, fields, dict(numel=numel, seeds=b.seeds.data_ptr()), status) for label, fields, numel, status in PLAN_ROWS]
    rows += [
        ("the plan's checks before the pointers", dict(noise_mode=2), dict(inputs=None), ERR_UNSUPPORTED),
        ("no operand array", dict(), dict(inputs=None), ERR_NULL),
        ("no out0", dict(), dict(out0=None), ERR_NULL),
        ("no out1", dict(out1_dtype=b.code), dict(), ERR_NULL),
        ("a missing output before a misaligned operand", dict(), dict(out0=None, inputs=b.ptrs(b.ops, **{"1": mis})), ERR_NULL),
        ("operand 1 missing", dict(), dict(inputs=b.ptrs(b.ops, **{"1": None})), ERR_NULL),
        ("operand 1 misaligned", dict(), dict(inputs=b.ptrs(b.ops, **{"1": mis})), ERR_ALIGN),
        ("operand 0 misaligned before operand 1 missing", dict(), dict(inputs=b.ptrs(b.ops, **{"0": mis, "1": None})), ERR_ALIGN),
        ("operand 0 missing before operand 1 misaligned", dict(), dict(inputs=b.ptrs(b.ops, **{"0": None, "1": mis})), ERR_NULL),
        ("a missing operand before a misaligned output", dict(), dict(inputs=b.ptrs(b.ops, **{"2": None}), out0=b.out0.data_ptr() + 2), ERR_NULL),
        ("out0 misaligned", dict(), dict(out0=b.out0.data_ptr() + 2), ERR_ALIGN),
        ("out1 misaligned", dict(out1_dtype=b.code), dict(out1=b.out1.data_ptr() + 2), ERR_ALIGN),
        ("alignment before the dtypes", dict(dtype_a=_hip.F64), dict(out0=b.out0.data_ptr() + 2), ERR_ALIGN),
        ("fp64 operands under fp32 arithmetic", dict(dtype_a=_hip.F64), dict(), ERR_DTYPE),
        ("no such dtype", dict(dtype_a=BAD), dict(), ERR_DTYPE),
        ("group b of another 16-bit dtype", dict(n_group_a=2, dtype_b=_hip.F16 if b.code != _hip.F16 else _hip.BF16), dict(), ERR_DTYPE),
        ("out0 of another 16-bit dtype", dict(out0_dtype=_hip.F16 if b.code != _hip.F16 else _hip.BF16), dict(), ERR_DTYPE),
        ("fp64 out0 under fp32 arithmetic", dict(out0_dtype=_hip.F64), dict(), ERR_DTYPE),
        ("out1 of neither the operands' dtype nor the wide one", dict(out1_dtype=_hip.F64), dict(out1=b.out1.data_ptr()), ERR_DTYPE),
        ("an empty batch", dict(), dict(numel=0), OK),
        ("an empty batch before the pointers", dict(), dict(numel=0, inputs=None, out0=None), OK),
        ("an empty batch asks for no sample size", dict(sample_numel=0, **NOISY), dict(numel=0, seeds=b.seeds.data_ptr()), OK),
    ]
    return rows


def kernarg_only_rows(b):
    return [
        ("fp32 group b under fp64 arithmetic", dict(acc_f64=1, n_group_a=2, dtype_b=_hip.F32), dict(), ERR_DTYPE if b.code != _hip.F32 else None),
        ("fp32 out0 under fp64 arithmetic", dict(acc_f64=1, out0_dtype=_hip.F32), dict(), ERR_DTYPE if b.code != _hip.F32 else None),
    ]


def run_step_table(b, entry, rows, extra=()):
    lib = _hip.load()
    fn = getattr(lib, entry)
    for label, fields, args, status in rows:
        if status is None:
            continue
        plan = step_plan(b, **fields) if fields is not None else None
        a = dict(inputs=b.ptrs(b.ops), out0=b.out0.data_ptr(), out1=None, seeds=None, numel=NUMEL, extra=extra)
        a.update(args)
        got = fn(ctypes.byref(plan) if plan is not None else None, a["inputs"], a["out0"], a["out1"], a["seeds"], a["numel"], *a["extra"], b.stream)
        assert got == status, (entry, label, got)
    assert b.untouched(), entry


def test_step_launch(bf, f32):
    for b in (bf, f32):
        run_step_table(b, "skr_step_launch", launch_rows(b) + kernarg_only_rows(b))
    lib = _hip.load()
    for b in (bf, f32):  # the controls
        assert lib.skr_step_launch(ctypes.byref(step_plan(b)), b.ptrs(b.ops), b.out0.data_ptr(), None, None, NUMEL, b.stream) == OK
        torch.cuda.synchronize()
        assert b.out0.any()
        b.out0.zero_()
    assert lib.skr_step_launch(ctypes.byref(step_plan(bf, **NOISY)), bf.ptrs(bf.ops), bf.out0.data_ptr(), None, bf.seeds.data_ptr(), NUMEL, bf.stream) == OK
    torch.cuda.synchronize()
    bf.out0.zero_()


FORMS = {"skr_step_launch_indexed": False, "skr_step_launch_indexed_per_sample": True, "skr_step_launch_rolling": True}


@pytest.mark.parametrize("entry", list(FORMS))
def test_table_forms(entry, bf, f32):
    per_sample = FORMS[entry]
    lib = _hip.load()
    for b in (bf, f32):
        table = (b.rows.data_ptr(), b.index.data_ptr(), 0)
        rows = [(label, fields, {**args, "extra": args.get("extra", table)}, status) for label, fields, args, status in launch_rows(b)]
        rows += [
            ("no table", dict(), dict(extra=(None, b.index.data_ptr(), 0)), ERR_NULL),
            ("no index", dict(), dict(extra=(b.rows.data_ptr(), None, 0)), ERR_NULL if per_sample else None),
            ("noise mode 1 without seeds, whatever the plan's zeta", dict(noise_mode=1), dict(extra=table), ERR_NULL),
            ("a negative row offset", dict(), dict(extra=(b.rows.data_ptr(), b.index.data_ptr(), -1)), ERR_UNSUPPORTED),
            ("fp64 arithmetic", dict(acc_f64=1), dict(extra=table), ERR_UNSUPPORTED),
            ("more operands than a row holds", dict(n_terms=17, n_group_a=17), dict(inputs=b.ptrs(b.ops + [b.ops[0]] * 14), extra=table), ERR_UNSUPPORTED),
            ("alignment before the table's checks", dict(), dict(out0=b.out0.data_ptr() + 2, extra=(b.rows.data_ptr(), b.index.data_ptr(), -1)), ERR_ALIGN),
            ("the table's checks before the dtypes", dict(dtype_a=_hip.F64), dict(extra=(b.rows.data_ptr(), b.index.data_ptr(), -1)), ERR_UNSUPPORTED),
            ("noise mode 1 over samples of no multiple of 8", dict(noise_mode=1, sample_numel=4), dict(seeds=b.seeds.data_ptr(), extra=table), ERR_UNSUPPORTED),
            ("noise mode 1 without a sample size", dict(noise_mode=1, sample_numel=0), dict(seeds=b.seeds.data_ptr(), extra=table), ERR_SHAPE),
            ("the sample size before the row offset", dict(noise_mode=1, sample_numel=0), dict(seeds=b.seeds.data_ptr(), extra=(b.rows.data_ptr(), b.index.data_ptr(), -1)), ERR_SHAPE),
            ("no whole chunk: no kernel reads a table", dict(sample_numel=1000), dict(numel=1000, extra=table), ERR_UNSUPPORTED),
            ("samples of half a chunk", dict(sample_numel=1024), dict(extra=table), ERR_UNSUPPORTED if per_sample else None),
            ("no sample size", dict(sample_numel=0), dict(extra=table), ERR_SHAPE if per_sample else None),
            ("samples that do not divide numel", dict(sample_numel=1000), dict(extra=table), ERR_SHAPE if per_sample else None),
        ]
        run_step_table(b, entry, rows)
    for b in (bf, f32):  # the controls
        fn = getattr(lib, entry)
        assert fn(ctypes.byref(step_plan(b)), b.ptrs(b.ops), b.out0.data_ptr(), None, None, NUMEL, b.rows.data_ptr(), b.index.data_ptr(), 0, b.stream) == OK
        torch.cuda.synchronize()
        assert b.out0.any()
        b.out0.zero_()


def test_program_create(bf, f32):
    lib = _hip.load()
    for b in (bf, f32):
        handle = ctypes.c_void_p()
        assert lib.skr_program_create(None, NUMEL, ctypes.byref(handle)) == ERR_NULL
        assert lib.skr_program_create(ctypes.byref(step_plan(b)), NUMEL, None) == ERR_NULL
        assert lib.skr_program_create(None, -1, None) == ERR_NULL
        for label, fields, numel, status in PLAN_ROWS:
            handle = ctypes.c_void_p(1)
            assert lib.skr_program_create(ctypes.byref(step_plan(b, **fields)), numel, ctypes.byref(handle)) == status, label
            assert handle.value is None, label  # (a refused plan leaves no handle behind)
        # what a launch checks, a program's creation does not: dtypes and pointers are the launch's business
        for fields, numel in ((dict(), NUMEL), (dict(dtype_a=BAD), NUMEL), (dict(sample_numel=0, **NOISY), 0)):
            assert lib.skr_program_create(ctypes.byref(step_plan(b, **fields)), numel, ctypes.byref(handle)) == OK, fields
            assert handle.value
            lib.skr_program_destroy(handle)
    assert bf.untouched() and f32.untouched()


def grad_plan(box, **fields):
    plan = _hip.StepGradPlanC()
    plan.n_grads = plan.n_group_a = N
    plan.dtype_a = plan.g0_dtype = box.code
    plan.dtype_b, plan.g1_dtype = _hip.F32, _hip.NONE
    for k in range(N):
        plan.a[k], plan.b[k] = 0.5 + k, 0.25
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def test_step_backward_launch(bf, f32):
    lib = _hip.load()
    for b in (bf, f32):
        g0, g1, mis = b.ops[0].data_ptr(), b.ops[1].data_ptr(), b.ops[0].data_ptr() + 2
        two = dict(g1_dtype=b.code)
        rows = [  # (label, plan fields, call arguments, status)
            ("no plan", None, dict(), ERR_NULL),
            ("no gradient", dict(n_grads=0, n_group_a=0), dict(), ERR_TERMS),
            ("more gradients than the maximum", dict(n_grads=81, n_group_a=81), dict(), ERR_TERMS),
            ("group a beyond the gradients", dict(n_group_a=4), dict(), ERR_TERMS),
            ("group a negative", dict(n_group_a=-1), dict(), ERR_TERMS),
            ("terms before numel", dict(n_grads=0, n_group_a=0), dict(numel=-1), ERR_TERMS),
            ("numel negative", dict(), dict(numel=-1), ERR_SHAPE),
            ("numel before the gradient array", dict(), dict(numel=-1, grads=None), ERR_SHAPE),
            ("no gradient array", dict(), dict(grads=None), ERR_NULL),
            ("the gradient array before the dtypes", dict(g0_dtype=BAD), dict(grads=None), ERR_NULL),
            ("no such g0 dtype", dict(g0_dtype=BAD), dict(), ERR_DTYPE),
            ("g0 dtype absent", dict(g0_dtype=_hip.NONE), dict(), ERR_DTYPE),
            ("no such g1 dtype", dict(g1_dtype=BAD), dict(g1=g1), ERR_DTYPE),
            ("no such dtype of group a", dict(dtype_a=BAD), dict(), ERR_DTYPE),
            ("no such dtype of group b", dict(n_group_a=2, dtype_b=BAD), dict(), ERR_DTYPE),
            ("the dtypes before the empty batch", dict(g0_dtype=BAD), dict(numel=0), ERR_DTYPE),
            ("an empty batch", dict(), dict(numel=0), OK),
            ("an empty batch before the pointers", dict(), dict(numel=0, g0=None), OK),
            ("no g0", dict(), dict(g0=None), ERR_NULL),
            ("a g1 dtype without g1", two, dict(), ERR_NULL),
            ("g1 without a g1 dtype", dict(), dict(g1=g1), ERR_NULL),
            ("a missing g1 before a misaligned g0", two, dict(g0=mis), ERR_NULL),
            ("g0 misaligned", dict(), dict(g0=mis), ERR_ALIGN),
            ("g1 misaligned", two, dict(g1=g1 + 2), ERR_ALIGN),
            ("a misaligned g0 before a missing gradient", dict(), dict(g0=mis, grads=b.ptrs(b.grads, **{"1": None})), ERR_ALIGN),
            ("gradient 1 missing", dict(), dict(grads=b.ptrs(b.grads, **{"1": None})), ERR_NULL),
            ("gradient 1 misaligned", dict(), dict(grads=b.ptrs(b.grads, **{"1": b.grads[1].data_ptr() + 2})), ERR_ALIGN),
            ("gradient 0 misaligned before gradient 1 missing", dict(), dict(grads=b.ptrs(b.grads, **{"0": b.grads[0].data_ptr() + 2, "1": None})), ERR_ALIGN),
            ("gradient 0 missing before gradient 1 misaligned", dict(), dict(grads=b.ptrs(b.grads, **{"0": None, "1": b.grads[1].data_ptr() + 2})), ERR_NULL),
        ]
        for label, fields, args, status in rows:
            plan = grad_plan(b, **fields) if fields is not None else None
            a = dict(g0=g0, g1=None, grads=b.ptrs(b.grads), numel=NUMEL)
            a.update(args)
            got = lib.skr_step_backward_launch(ctypes.byref(plan) if plan is not None else None, a["g0"], a["g1"], a["grads"], a["numel"], b.stream)
            assert got == status, (label, got)
        assert b.untouched()
        assert lib.skr_step_backward_launch(ctypes.byref(grad_plan(b)), g0, None, b.ptrs(b.grads), NUMEL, b.stream) == OK  # the control
        torch.cuda.synchronize()
        assert all(g.any() for g in b.grads)
        for g in b.grads:
            g.zero_()


def test_error_mean(bf, f32):
    lib = _hip.load()
    for b in (bf, f32):
        x, y, out, part = b.ops[0].data_ptr(), b.ops[1].data_ptr(), b.scalar.data_ptr(), b.partials.data_ptr()
        rows = [  # (label, (a, b, dtype, numel, power, out, partials), status)
            ("no b", (x, None, b.code, NUMEL, 1, out, part), ERR_NULL),
            ("no result", (x, y, b.code, NUMEL, 1, None, part), ERR_NULL),
            ("no partials", (x, y, b.code, NUMEL, 1, out, None), ERR_NULL),
            ("the pointers before numel", (x, None, b.code, 0, 1, out, part), ERR_NULL),
            ("an empty tensor has no mean", (x, y, b.code, 0, 1, out, part), ERR_SHAPE),
            ("numel negative", (x, y, b.code, -1, 2, out, part), ERR_SHAPE),
            ("numel before the power", (x, y, b.code, 0, 3, out, part), ERR_SHAPE),
            ("power 3", (x, y, b.code, NUMEL, 3, out, part), ERR_UNSUPPORTED),
            ("power 0", (None, y, b.code, NUMEL, 0, out, part), ERR_UNSUPPORTED),
            ("the power before the dtype", (x, y, BAD, NUMEL, 3, out, part), ERR_UNSUPPORTED),
            ("no such dtype", (x, y, BAD, NUMEL, 1, out, part), ERR_DTYPE),
            ("dtype absent", (x, y, _hip.NONE, NUMEL, 2, out, part), ERR_DTYPE),
        ]
        for label, args, status in rows:
            assert lib.skr_error_mean(*args, b.stream) == status, label
        assert b.untouched() and not b.partials.any()
        for a_ptr in (x, None):  # the controls: a may be absent (= zeros)
            assert lib.skr_error_mean(a_ptr, y, b.code, NUMEL, 1, out, part, b.stream) == OK
        torch.cuda.synchronize()
        assert b.scalar.item() > 0
        b.scalar.zero_()
        b.partials.zero_()


def test_power_blend(bf, f32):
    lib = _hip.load()
    for b in (bf, f32):
        x, y, out, c = b.ops[0].data_ptr(), b.ops[1].data_ptr(), b.wide.data_ptr(), b.code
        rows = [  # (label, (out, out_dtype, a, a_dtype, b, b_dtype, p, c, power, numel), status)
            ("numel negative", (out, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, -1), ERR_SHAPE),
            ("numel before the pointers", (None, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, -1), ERR_SHAPE),
            ("an empty tensor", (out, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, 0), OK),
            ("an empty tensor before the pointers, the power and the dtypes", (None, BAD, None, BAD, None, BAD, 0.5, 0.5, 0.0, 0), OK),
            ("no out", (None, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_NULL),
            ("no a", (out, _hip.F32, None, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_NULL),
            ("no b", (out, _hip.F32, x, c, None, c, 0.5, 0.5, 2.0, NUMEL), ERR_NULL),
            ("the pointers before the power", (out, _hip.F32, None, c, y, c, 0.5, 0.5, 0.0, NUMEL), ERR_NULL),
            ("power 0", (out, _hip.F32, x, c, y, c, 0.5, 0.5, 0.0, NUMEL), ERR_UNSUPPORTED),
            ("the power before the dtypes", (out, _hip.BF16, x, c, y, c, 0.5, 0.5, 0.0, NUMEL), ERR_UNSUPPORTED),
            ("a 16-bit result", (out, _hip.BF16, x, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("no such result dtype", (out, BAD, x, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("no such dtype of a", (out, _hip.F32, x, BAD, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("no such dtype of b", (out, _hip.F32, x, c, y, BAD, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("dtype of b absent", (out, _hip.F32, x, c, y, _hip.NONE, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
        ]
        for label, args, status in rows:
            assert lib.skr_power_blend(*args, b.stream) == status, label
        assert b.untouched()
        assert lib.skr_power_blend(out, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, NUMEL, b.stream) == OK  # the control
        torch.cuda.synchronize()
        assert b.wide.any()
        b.wide.zero_()


def test_power_blend_backward(bf, f32):
    lib = _hip.load()
    for b in (bf, f32):
        x, y, c = b.ops[0].data_ptr(), b.ops[1].data_ptr(), b.code
        ga, gb = b.grads[0].data_ptr(), b.grads[1].data_ptr()
        g = torch.ones(NUMEL, dtype=torch.float32, device=b.dev)
        gp = g.data_ptr()
        rows = [  # (label, (grad_a, grad_b, g, g_dtype, a, a_dtype, b, b_dtype, p, c, power, numel), status)
            ("numel negative", (ga, gb, gp, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, -1), ERR_SHAPE),
            ("numel before the pointers", (ga, gb, None, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, -1), ERR_SHAPE),
            ("an empty tensor before everything else", (ga, gb, None, BAD, None, BAD, None, BAD, 0.5, 0.5, 0.0, 0), OK),
            ("no gradient asked for, before everything else", (None, None, None, BAD, None, BAD, None, BAD, 0.5, 0.5, 0.0, NUMEL), OK),
            ("no g", (ga, gb, None, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_NULL),
            ("no a", (ga, None, gp, _hip.F32, None, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_NULL),
            ("no b", (None, gb, gp, _hip.F32, x, c, None, c, 0.5, 0.5, 2.0, NUMEL), ERR_NULL),
            ("the pointers before the power", (ga, gb, None, _hip.F32, x, c, y, c, 0.5, 0.5, 0.0, NUMEL), ERR_NULL),
            ("power 0", (ga, gb, gp, _hip.F32, x, c, y, c, 0.5, 0.5, 0.0, NUMEL), ERR_UNSUPPORTED),
            ("the power before the dtypes", (ga, gb, gp, _hip.BF16, x, c, y, c, 0.5, 0.5, 0.0, NUMEL), ERR_UNSUPPORTED),
            ("a 16-bit incoming gradient", (ga, gb, gp, _hip.BF16, x, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("no such dtype of g", (ga, gb, gp, BAD, x, c, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("no such dtype of a", (ga, gb, gp, _hip.F32, x, BAD, y, c, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
            ("no such dtype of b", (ga, gb, gp, _hip.F32, x, c, y, BAD, 0.5, 0.5, 2.0, NUMEL), ERR_DTYPE),
        ]
        for label, args, status in rows:
            assert lib.skr_power_blend_backward(*args, b.stream) == status, label
        assert b.untouched()
        assert lib.skr_power_blend_backward(ga, gb, gp, _hip.F32, x, c, y, c, 0.5, 0.5, 2.0, NUMEL, b.stream) == OK  # the control
        torch.cuda.synchronize()
        assert b.grads[0].any() and b.grads[1].any()
        for t in b.grads:
            t.zero_()


def test_noise_random(bf, f32):
    lib = _hip.load()
    for b in (bf, f32):
        out, seeds = b.out0.data_ptr(), b.seeds.data_ptr()
        rows = [  # (label, (out, out_dtype, seeds, stream_id, batch, sample_numel), status)
            ("batch negative", (out, b.code, seeds, 3, -1, NUMEL), ERR_SHAPE),
            ("sample size negative", (out, b.code, seeds, 3, 1, -1), ERR_SHAPE),
            ("the sizes before the pointers", (None, b.code, seeds, 3, -1, NUMEL), ERR_SHAPE),
            ("a negative size before an empty one", (out, b.code, seeds, 3, 0, -1), ERR_SHAPE),
            ("an empty batch before the pointers and the dtype", (None, BAD, None, 3, 0, NUMEL), OK),
            ("empty samples", (out, b.code, seeds, 3, 1, 0), OK),
            ("no out", (None, b.code, seeds, 3, 1, NUMEL), ERR_NULL),
            ("no seeds", (out, b.code, None, 3, 1, NUMEL), ERR_NULL),
            ("the pointers before the dtype", (None, BAD, seeds, 3, 1, NUMEL), ERR_NULL),
            ("no such dtype", (out, BAD, seeds, 3, 1, NUMEL), ERR_DTYPE),
            ("dtype absent", (out, _hip.NONE, seeds, 3, 1, NUMEL), ERR_DTYPE),
        ]
        for label, args, status in rows:
            assert lib.skr_noise_random(*args, b.stream) == status, label
        assert b.untouched()
        assert lib.skr_noise_random(out, b.code, seeds, 3, 1, NUMEL, b.stream) == OK  # the control
        torch.cuda.synchronize()
        assert b.out0.any()
        b.out0.zero_()


# ---- the Pyramid generators: 2 samples of a 256-element unit, bf16 ----------------------------------------------------------------------------
# Every row but the dtype rows is refused before anything is launched.  The generators learn their output dtype last, in pass 2: a
# call that is well formed but for its dtype runs pass 1 on its (valid) workspaces and leaves `out` alone, so those rows carry whole
# buffers.  Rows that name a shape beyond the buffers are refused by the check they pin, ahead of any launch.
PYR_BATCH, PYR_UNIT = 2, 256
PYR_POINTERS = {"skr_noise_pyramid": ("out", "scratch", "partials", "table", "seeds"), "skr_noise_pyramid_any": ("out", "scratch", "normals", "partials", "table", "seeds")}
PYR_POINTERS["skr_noise_pyramid_nd"] = PYR_POINTERS["skr_noise_pyramid_any"]


class PyramidBox:
    def __init__(self, dev):
        self.out = torch.zeros(PYR_BATCH * PYR_UNIT, dtype=torch.bfloat16, device=dev)
        self.scratch, self.normals = (torch.zeros(PYR_BATCH * PYR_UNIT, dtype=torch.float32, device=dev) for _ in range(2))
        self.partials = torch.zeros(PYR_BATCH * 2, dtype=torch.float64, device=dev)  # one pair per sample: lead = 1, n_slots = 1
        self.table = torch.zeros(PYR_BATCH * 17, dtype=torch.int32, device=dev)
        self.seeds = torch.tensor([11, 12], dtype=torch.int64, device=dev)
        self.stream = _hip.current_stream_ptr(dev)

    def call(self, entry, **change):
        "the well-formed call of `entry` with `change` applied: a pointer's name -> None, or an argument's name -> its value"
        a = dict(dtype=_hip.BF16, n_slots=1, batch=PYR_BATCH, lead=1, h=16, w=16, resize_h=1, depth=99, nd=3, shape=(8, 2, 16), axis_a=0, axis_b=2)
        a.update({name: getattr(self, name).data_ptr() for name in PYR_POINTERS[entry]})
        assert not set(change) - set(a), change
        a.update(change)
        lib = _hip.load()
        tail = (0.3, a["depth"], 1, self.stream)
        if entry == "skr_noise_pyramid":
            return lib.skr_noise_pyramid(a["out"], a["dtype"], a["scratch"], a["partials"], a["table"], a["seeds"], 0, 0, a["batch"], a["lead"], a["h"], a["w"], a["resize_h"], *tail)
        head = (a["out"], a["dtype"], a["scratch"], a["normals"], a["partials"], a["n_slots"], a["table"], a["seeds"], 0, 0, a["batch"])
        if entry == "skr_noise_pyramid_any":
            return lib.skr_noise_pyramid_any(*head, a["lead"], a["h"], a["w"], a["resize_h"], *tail)
        shape = None if a["shape"] is None else (ctypes.c_int64 * len(a["shape"]))(*a["shape"])
        return lib.skr_noise_pyramid_nd(*head, a["nd"], shape, a["axis_a"], a["axis_b"], *tail)

    def run(self, entry, rows, controls):
        for label, change, status in rows:
            assert self.call(entry, **change) == status, (entry, label)
        torch.cuda.synchronize()
        assert not self.out.any(), entry
        for change in controls:
            assert self.call(entry, **change) == OK, (entry, change)
            torch.cuda.synchronize()
            assert self.out.any(), (entry, change)
            self.out.zero_()


@pytest.fixture(scope="module")
def pyr(dev):
    return PyramidBox(dev)


def null_rows(entry):
    nothing = {name: None for name in PYR_POINTERS[entry]}
    return [("an empty batch before the pointers and the dtype", dict(batch=0, dtype=BAD, **nothing), OK)] + [(f"no {name}", {name: None}, ERR_NULL) for name in nothing]


def test_noise_pyramid(pyr):
    rows = [  # (label, what differs from the well-formed call, status)
        ("batch negative", dict(batch=-1), ERR_SHAPE),
        ("no leading slice", dict(lead=0), ERR_SHAPE),
        ("no row", dict(h=0), ERR_SHAPE),
        ("no column", dict(w=0), ERR_SHAPE),
        ("depth negative", dict(depth=-1), ERR_SHAPE),
        ("the sizes before the empty batch", dict(batch=0, lead=0), ERR_SHAPE),
        ("the sizes before the pointers", dict(out=None, depth=-1), ERR_SHAPE),
        ("an empty batch before the width", dict(batch=0, w=18), OK),
        *null_rows("skr_noise_pyramid"),
        ("the pointers before the width", dict(seeds=None, w=18), ERR_NULL),
        ("a width of no multiple of 4", dict(w=18), ERR_UNSUPPORTED),
        ("h above 32767", dict(h=32768), ERR_UNSUPPORTED),
        ("w above 32767", dict(w=32768), ERR_UNSUPPORTED),
        ("the width before the rows of a unit without resized rows", dict(resize_h=0, h=2, w=18), ERR_UNSUPPORTED),
        ("the sides before the rows of a unit without resized rows", dict(resize_h=0, h=32768), ERR_UNSUPPORTED),
        ("rows without resized rows", dict(resize_h=0, h=2), ERR_SHAPE),
        ("rows without resized rows before the batch", dict(resize_h=0, h=2, batch=65536), ERR_SHAPE),
        ("batch above 65535", dict(batch=65536), ERR_UNSUPPORTED),
        ("more than 2^31 - 1 slices", dict(lead=1 << 31), ERR_UNSUPPORTED),
        ("the level stage: 42 708 floats for 38 * 1024", dict(h=400, w=400), ERR_UNSUPPORTED),
        ("the level stage at its edge", dict(h=384, w=380), ERR_UNSUPPORTED),
        ("the level stage before the dtype", dict(h=400, w=400, dtype=BAD), ERR_UNSUPPORTED),
        ("no such dtype", dict(dtype=BAD), ERR_DTYPE),
        ("dtype absent", dict(dtype=_hip.NONE), ERR_DTYPE),
    ]
    pyr.run("skr_noise_pyramid", rows, [dict(), dict(resize_h=0, h=1, w=256)])


ND_ROWS = [  # the checks of the any-shape kernels, shared by skr_noise_pyramid_any and skr_noise_pyramid_nd
    ("batch negative", dict(batch=-1), ERR_SHAPE),
    ("depth negative", dict(depth=-1), ERR_SHAPE),
    ("no partial slot", dict(n_slots=0), ERR_SHAPE),
    ("the counts before the empty batch", dict(batch=0, n_slots=0), ERR_SHAPE),
    ("the counts before the pointers", dict(out=None, depth=-1), ERR_SHAPE),
    ("batch above 65535", dict(batch=65536), ERR_UNSUPPORTED),
    ("more than 65535 partial slots", dict(n_slots=65536), ERR_UNSUPPORTED),
    ("the pointers before the limits", dict(table=None, n_slots=65536), ERR_NULL),
    ("the limits before the dtype", dict(n_slots=65536, dtype=BAD), ERR_UNSUPPORTED),
    ("no such dtype", dict(dtype=BAD), ERR_DTYPE),
    ("dtype absent", dict(dtype=_hip.NONE), ERR_DTYPE),
]


def test_noise_pyramid_any(pyr):
    rows = [
        ("no leading slice", dict(lead=0), ERR_SHAPE),
        ("no row", dict(h=0), ERR_SHAPE),
        ("no column", dict(w=0), ERR_SHAPE),
        ("rows without resized rows", dict(resize_h=0, h=2), ERR_SHAPE),
        ("the sizes before the empty batch", dict(batch=0, resize_h=0, h=2), ERR_SHAPE),
        ("more than 2^31 - 1 slices", dict(lead=1 << 31), ERR_SHAPE),
        *null_rows("skr_noise_pyramid_any"),
        *ND_ROWS,
        ("h above 32767", dict(h=32768), ERR_UNSUPPORTED),
        ("w above 32767", dict(w=32768), ERR_UNSUPPORTED),
    ]
    pyr.run("skr_noise_pyramid_any", rows, [dict(), dict(h=14, w=18), dict(resize_h=0, h=1, w=250)])


def test_noise_pyramid_nd(pyr):
    rows = [
        ("no axis", dict(nd=0), ERR_SHAPE),
        ("five axes", dict(nd=5), ERR_SHAPE),
        ("no shape", dict(shape=None), ERR_SHAPE),
        ("the axis count before the empty batch", dict(batch=0, nd=0), ERR_SHAPE),
        ("axis b negative", dict(axis_b=-1), ERR_SHAPE),
        ("axis b beyond the unit", dict(axis_b=3), ERR_SHAPE),
        ("axis a not ahead of axis b", dict(axis_a=2), ERR_SHAPE),
        ("axis a below -1", dict(axis_a=-2), ERR_SHAPE),
        ("the axes before the empty batch", dict(batch=0, axis_a=2), ERR_SHAPE),
        ("an empty axis", dict(shape=(8, 0, 16)), ERR_SHAPE),
        ("an axis of 2^31", dict(shape=(1 << 31, 2, 16)), ERR_SHAPE),
        ("the shape before the pointers", dict(out=None, shape=(8, 0, 16)), ERR_SHAPE),
        *null_rows("skr_noise_pyramid_nd"),
        *ND_ROWS,
        ("h above 32767", dict(shape=(32768, 2, 16)), ERR_UNSUPPORTED),
        ("w above 32767", dict(shape=(8, 2, 32768)), ERR_UNSUPPORTED),
        ("more than 2^31 - 1 slices", dict(shape=((1 << 31) - 1, 2, 16), axis_a=-1), ERR_UNSUPPORTED),
    ]
    pyr.run("skr_noise_pyramid_nd", rows, [dict(), dict(axis_a=-1), dict(nd=2, shape=(16, 16), axis_a=0, axis_b=1)])
