"""The launch table against the real ABI (needs an MI355X): for every (kind, form) key of `_hip.ENTRIES`, one launch laid out by the table
(`_hip.call_entry`) and one through `getattr(lib, name)` with the arguments written out by hand below, on the same inputs.  Both run the
same kernel on the same data, so the comparison is bitwise; there is no tolerance to choose.  A stub cannot prove the argument ORDER: two
pointers swapped, or numel where the row offset belongs, change what the kernel writes -- or make the entry refuse the call.
What this proves is the ORDER the rule gives every entry.  The names under which the real launchers file their values (`launch_call`,
`IndexedRows.launch`, `RollingBatch._launch`) are covered by the suites of those launchers: the values dict here is the test's own.

Shapes, the smallest the row kernels take: bf16, 2 samples of 2048 elements (one chunk per sample), 3 operands, a one-row table read by
both samples (index = [0, 0], row_offset 0), a mask of 8 elements per sample, a channels-last layout of (4, 512).  noise_mode is 0, except
for one drawing case per form (the plain kind) with fixed seeds."""

import ctypes

import pytest
import torch

from skrample_amd import _hip

pytestmark = pytest.mark.gpu
SAMPLES, SAMPLE, OPERANDS, MASK, LAYOUT = 2, 2048, 3, 8, (4, 512)
NUMEL = SAMPLES * SAMPLE
COEF0, COEF1, ZETA, STREAM, SCALE, PHI, SLOT = (0.5, -0.25, 1.5), (0.25, 0.75, -0.5), 0.45, 3 * 256, 7.3, 0.7, 1
KEYS = sorted(_hip.ENTRIES)
NOISY = [("plain", form) for form in _hip.FORMS]


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs(dev):
    "the tensors every case reads, made once and never written: operands, cond, mask, factor, seeds, the index and the one-row table"
    g = torch.Generator().manual_seed(2210)
    draw = lambda *shape: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    row = _hip.StepRowC()
    for k in range(OPERANDS):
        row.coef0[k], row.coef1[k] = COEF0[k], COEF1[k]
    row.zeta0, row.stream0 = ZETA, STREAM
    row.convert_k[0], row.convert_k[1] = SCALE, PHI
    rows = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
    _hip.upload_rows(rows, 0, [row])
    return dict(ops=[draw(SAMPLES, SAMPLE) for _ in range(OPERANDS)], cond=draw(SAMPLES, SAMPLE), mask=(torch.rand((SAMPLES, MASK), generator=g) < 0.5).bfloat16().to(dev),
                factor=torch.tensor([0.75, 1.25], dtype=torch.bfloat16, device=dev), seeds=torch.tensor([11, 22], dtype=torch.int64, device=dev),
                index=torch.zeros(SAMPLES, dtype=torch.int32, device=dev), rows=rows)  # fmt: skip


def make_plan(kind, form, noisy):
    "the plan of a case: a table form gets its scalars from the row, and other, non-zero ones here, which it must ignore"
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = OPERANDS
    plan.dtype_a = plan.out0_dtype = _hip.BF16
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.sample_numel, plan.noise_mode = SAMPLE, 1 if noisy else 0
    table = form in _hip.FORMS[2:]
    for k in range(OPERANDS):
        plan.coef0[k] = 9.0 + k if table else COEF0[k]
        plan.coef1[k] = (-7.0 - k if table else COEF1[k]) if kind == "masked" else 0.0
    if noisy:
        plan.zeta0, plan.stream0 = (5.0, 77) if table else (ZETA, STREAM)
    return plan


def bits(t):
    return t.view(torch.int16)


CASES = [(kind, form, False) for kind, form in KEYS] + [(kind, form, True) for kind, form in NOISY]


@pytest.mark.parametrize("kind,form,noisy", CASES, ids=[f"{kind}-{form}{'-noisy' if noisy else ''}" for kind, form, noisy in CASES])
def test_a_launch_through_the_table_equals_the_launch_written_out_by_hand(kind, form, noisy, dev, inputs):
    lib = _hip.load()
    name = _hip.entry_name(kind, form)
    ops, cond, factor_in = inputs["ops"], inputs["cond"], inputs["factor"]
    arr = (ctypes.c_void_p * OPERANDS)(*[t.data_ptr() for t in ops])
    plan = make_plan(kind, form, noisy)
    mask = _hip.StepMaskC(inputs["mask"].data_ptr(), _hip.BF16, 0, MASK, MASK)
    layout = _hip.StepLayoutC(*LAYOUT)
    seeds = inputs["seeds"].data_ptr() if noisy else None
    rows, index, stream = inputs["rows"].data_ptr(), inputs["index"].data_ptr(), _hip.current_stream_ptr(dev)
    uncond = ops[SLOT].data_ptr()
    # poisoned with ones: [0] is written through the table, [1] by hand
    outs = [torch.ones(SAMPLES, SAMPLE, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    stored = [torch.ones(SAMPLES, SAMPLE, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    factors = [torch.ones(SAMPLES, dtype=torch.bfloat16, device=dev) for _ in range(2)]
    partials = torch.zeros(_hip.guidance_partials(NUMEL, SAMPLE), dtype=torch.float64, device=dev)
    guides = [_hip.StepGuidanceC(cond.data_ptr(), s.data_ptr(), SCALE, SLOT, 0) for s in stored]
    rescale = _hip.StepRescaleC(factor_in.data_ptr(), PHI, SAMPLE, 0)

    values = dict(plan=plan, operands=arr, out0=outs[0].data_ptr(), out1=None, mask=mask, guide=guides[0], rescale=rescale, seeds=seeds, layout=layout, numel=NUMEL, rows=rows,
                  index=index, row_offset=0, stream=stream, uncond=uncond, cond=cond.data_ptr(), dtype=_hip.BF16, scale=SCALE, sample_numel=SAMPLE, factor=factors[0].data_ptr(),
                  stats=None, partials=partials.data_ptr())  # fmt: skip
    status = _hip.call_entry(lib, kind, form, values)
    assert status == 0, (name, status)

    P, M, G, R, L = (ctypes.byref(s) for s in (plan, mask, guides[1], rescale, layout))
    out, fac, part, c = outs[1].data_ptr(), factors[1].data_ptr(), partials.data_ptr(), cond.data_ptr()
    by_hand = {
        "skr_step_launch": (P, arr, out, None, seeds, NUMEL, stream),
        "skr_step_launch_channels_last": (P, arr, out, None, seeds, L, NUMEL, stream),
        "skr_step_launch_indexed": (P, arr, out, None, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_indexed_per_sample": (P, arr, out, None, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_rolling": (P, arr, out, None, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_masked": (P, arr, out, M, seeds, NUMEL, stream),
        "skr_step_launch_masked_channels_last": (P, arr, out, M, seeds, L, NUMEL, stream),
        "skr_step_launch_masked_indexed": (P, arr, out, M, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_masked_indexed_per_sample": (P, arr, out, M, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_masked_rolling": (P, arr, out, M, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_guided": (P, arr, out, G, seeds, NUMEL, stream),
        "skr_step_launch_guided_indexed": (P, arr, out, G, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_guided_indexed_per_sample": (P, arr, out, G, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_guided_rolling": (P, arr, out, G, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_guided_rescaled": (P, arr, out, G, R, seeds, NUMEL, stream),
        "skr_step_launch_guided_rescaled_indexed": (P, arr, out, G, R, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_guided_rescaled_indexed_per_sample": (P, arr, out, G, R, seeds, NUMEL, rows, index, 0, stream),
        "skr_step_launch_guided_rescaled_rolling": (P, arr, out, G, R, seeds, NUMEL, rows, index, 0, stream),
        "skr_guidance_rescale_factor": (uncond, c, _hip.BF16, SCALE, NUMEL, SAMPLE, fac, None, part, stream),
        "skr_guidance_rescale_factor_indexed": (uncond, c, _hip.BF16, NUMEL, SAMPLE, rows, index, 0, fac, None, part, stream),
        "skr_guidance_rescale_factor_indexed_per_sample": (uncond, c, _hip.BF16, NUMEL, SAMPLE, rows, index, 0, fac, None, part, stream),
        "skr_guidance_rescale_factor_rolling": (uncond, c, _hip.BF16, NUMEL, SAMPLE, rows, index, 0, fac, None, part, stream),
    }
    assert len(by_hand) == len(_hip.ENTRIES) == 22
    status = getattr(lib, name)(*by_hand[name])
    assert status == 0, (name, status)
    torch.cuda.synchronize(dev)

    ones = torch.ones_like(outs[0])
    if kind == _hip.FACTOR:
        assert torch.equal(bits(factors[0]), bits(factors[1])) and not torch.equal(factors[0], torch.ones_like(factors[0])), (name, factors)
        assert torch.equal(outs[0], ones) and torch.equal(outs[1], ones)  # the statistic writes the factor, nothing else
        return
    assert torch.equal(bits(outs[0]), bits(outs[1])), (name, int((bits(outs[0]) != bits(outs[1])).sum()))
    assert not torch.equal(outs[0], ones), name  # the launch wrote its output
    if kind in ("guided", "guided_rescaled"):
        assert torch.equal(bits(stored[0]), bits(stored[1])) and not torch.equal(stored[0], ones), name
    if noisy:  # the draw took part: the quiet launch of the same case writes something else
        quiet = torch.ones_like(outs[0])
        status = _hip.call_entry(lib, kind, form, dict(values, plan=make_plan(kind, form, False), out0=quiet.data_ptr(), seeds=None))
        assert status == 0 and not torch.equal(bits(quiet), bits(outs[0])), name
