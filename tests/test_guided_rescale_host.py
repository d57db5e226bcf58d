"""Rescaled guidance (guidance_rescale) without a device: the two C ABI declarations, their bindings and their checks,
lazy.Guidance(..., rescale=) and SkrampleWrapperScheduler.step_guided(..., guidance_rescale=) on CPU tensors, and the refusals.

The contract is one sentence -- a rescaled guided step returns the bits of the pipeline's three guidance lines, diffusers' four
rescale_noise_cfg lines and step() -- so every comparison is made on the integer views of the bits.  Host-resident operands evaluate the
lines with torch itself: equality is by construction, and what is tested is that the new keyword reaches them and that the wrapper's
bookkeeping stays that of step()."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, graphs
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR, STEP = "skr_guidance_rescale_factor", "skr_step_launch_guided_rescaled"
FIELDS = ["factor_dev", "phi", "sample_numel", "reserved"]
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def same_bits(a, b):
    a, b = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (a, b))  # (pred_original_sample may be lazy)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype]))


def diffusers_lines(u, c, g, phi):
    "the pipeline's three guidance lines and rescale_noise_cfg, written out"
    p = u + g * (c - u)
    std_text = c.std(dim=list(range(1, c.ndim)), keepdim=True)
    std_cfg = p.std(dim=list(range(1, p.ndim)), keepdim=True)
    resc = p * (std_text / std_cfg)
    return phi * resc + (1 - phi) * p


def test_header_declares_both_entries_and_the_struct_and_the_abi_is_still_15():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"int\s+skr_guidance_rescale_factor\s*\(\s*const\s+void\s*\*\s*uncond,\s*const\s+void\s*\*\s*cond,\s*int32_t\s+dtype,\s*double\s+scale,\s*int64_t\s+numel,\s*int64_t\s+sample_numel,", header)
    assert re.search(r"int\s+skr_step_launch_guided_rescaled\s*\(\s*const\s+skr_step_plan\s*\*\s*plan,\s*const\s+void\s*\*\s*const\s*\*\s*inputs,\s*void\s*\*\s*out,\s*const\s+skr_step_guidance\s*\*\s*guide,\s*const\s+skr_step_rescale\s*\*", header)
    body = re.search(r"typedef\s+struct\s+skr_step_rescale\s*\{(.*?)\}\s*skr_step_rescale\s*;", header, re.S)
    assert body is not None
    assert re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15
    for name in (FACTOR, STEP):
        assert name in _hip.EXPORTS
    assert callable(_hip.launch_guidance_factor) and callable(_hip.launch_step_guided_rescaled)
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    assert len(getattr(lib, FACTOR).argtypes) == 10 and len(getattr(lib, STEP).argtypes) == 8


def test_binding_struct_and_workspace_formula_match_the_header(tmp_path):
    assert [name for name, _ in _hip.StepRescaleC._fields_] == FIELDS
    want = {"factor_dev": 0, "phi": 8, "sample_numel": 16, "reserved": 24}
    assert {name: getattr(_hip.StepRescaleC, name).offset for name in FIELDS} == want and ctypes.sizeof(_hip.StepRescaleC) == 32
    sizes = [(6144, 2048), (800, 400), (600, 300), (8, 8), (131072, 65536), (2 * 2049, 2049)]
    assert [_hip.guidance_partials(n, sn) for n, sn in sizes] == [12, 8, 8, 4, 256, 16]
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "layout.c"
    checks = "".join(f'_Static_assert(offsetof(skr_step_rescale, {name}) == {off}, "{name}");\n' for name, off in want.items())
    checks += "".join(f'_Static_assert(SKR_GUIDANCE_PARTIALS({n}, {sn}) == {_hip.guidance_partials(n, sn)}, "partials");\n' for n, sn in sizes)
    src.write_text(f'#include <stddef.h>\n#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n{checks}_Static_assert(sizeof(skr_step_rescale) == 32, "size");\nint main(void) {{ return 0; }}\n')
    done = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_a_plain_c_client_compiles(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        "int main(void) {\n"
        "  skr_step_rescale rescale = {0, 0.7, 65536, 0};\n"
        "  int (*stat)(const void*, const void*, int32_t, double, int64_t, int64_t, void*, double*, double*, void*) = skr_guidance_rescale_factor;\n"
        "  int (*launch)(const skr_step_plan*, const void* const*, void*, const skr_step_guidance*, const skr_step_rescale*, const uint64_t*, int64_t, void*) =\n"
        "      skr_step_launch_guided_rescaled;\n"
        "  (void)rescale; (void)stat; (void)launch;\n"
        f"  return SKR_ABI_VERSION == {_hip.ABI_VERSION} && SKR_GUIDANCE_PARTIALS(131072, 65536) == 256 ? 0 : 1;\n"
        "}\n"
    )
    done = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "client.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_the_statistic_checks_answer_before_any_pointer_is_dereferenced_and_in_order():
    entry = getattr(_hip.load(), FACTOR)
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15
    u, c, factor, stats, partials = (base + 32 * k for k in range(5))

    def call(u=u, c=c, dtype=_hip.BF16, scale=7.5, numel=8192, sample_numel=4096, factor=factor, stats=stats, partials=partials):
        return entry(u, c, dtype, scale, numel, sample_numel, factor, stats, partials, None)

    table = [
        ("no uncond", dict(u=None), NULL),
        ("no cond", dict(c=None), NULL),
        ("no factor", dict(factor=None), NULL),
        ("no partials", dict(partials=None), NULL),
        ("negative numel", dict(numel=-8), SHAPE),
        ("samples of one element", dict(sample_numel=1), SHAPE),
        ("samples of no element", dict(sample_numel=0), SHAPE),
        ("samples that do not divide the launch", dict(sample_numel=4095), SHAPE),
        ("empty launch", dict(numel=0), OK),
        ("empty launch, no stats", dict(numel=0, stats=None), OK),
        ("a misaligned uncond", dict(u=u + 2), ALIGN),
        ("a misaligned cond", dict(c=c + 8), ALIGN),
        ("a dtype code that names none", dict(dtype=9), DTYPE),
        ("no dtype", dict(dtype=_hip.NONE), DTYPE),
        # two faults: the earlier check answers
        ("no cond + negative numel", dict(c=None, numel=-1), NULL),
        ("sample size + misaligned", dict(sample_numel=1, u=u + 2), SHAPE),
        ("empty + misaligned + dtype", dict(numel=0, u=u + 2, dtype=9), OK),
        ("misaligned + dtype", dict(c=c + 4, dtype=9), ALIGN),
    ]
    for what, kwargs, want in table:
        assert call(**kwargs) == want, what
    assert bytes(buf) == bytes(256)  # nothing was written


def make_plan(**fields):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.out0_dtype = _hip.BF16
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.coef0[0], plan.coef0[1] = 1.0, -0.5
    plan.sample_numel = 4096
    plan.noise_mode, plan.zeta0, plan.stream0 = 1, 0.5, 256
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def test_the_step_checks_are_those_of_the_guided_launch_with_the_rescale_among_them_in_order():
    "host buffers that are never read stand in for device pointers: every status below is returned ahead of the launch"
    entry = getattr(_hip.load(), STEP)
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, out, cond, gout, seeds, factor = (base + 32 * k for k in range(7))

    def call(plan=None, inputs=(a, b), out=out, cond=cond, gout=gout, scale=7.5, slot=1, reserved=0, seeds=seeds, numel=8192, factor=factor, phi=0.7, stat_numel=4096,
             rs_reserved=0, no_plan=False, no_guide=False, no_rescale=False, no_inputs=False):
        plan = plan if plan is not None else make_plan()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, scale, slot, reserved)
        rescale = _hip.StepRescaleC(factor, phi, stat_numel, rs_reserved)
        return entry(None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide),
                     None if no_rescale else ctypes.byref(rescale), seeds, numel, None)

    quiet = dict(noise_mode=0, zeta0=0.0)  # a plan that does not draw
    table = [
        # skr_step_launch_guided's, in its order
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("no rescale", dict(no_rescale=True), NULL),
        ("a draw without seeds", dict(seeds=None), NULL),
        ("too many operands", dict(plan=make_plan(n_terms=17, n_group_a=17)), TERMS),
        ("slot beyond the operands", dict(slot=2), TERMS),
        ("negative numel", dict(numel=-8), SHAPE),
        ("no output at all", dict(plan=make_plan(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a,), out=None, gout=None, slot=0), NULL),
        ("noise_mode 2", dict(plan=make_plan(noise_mode=2)), UNSUPPORTED),
        ("a second output", dict(plan=make_plan(out1_dtype=_hip.BF16)), UNSUPPORTED),
        ("the guide's reserved", dict(reserved=1), UNSUPPORTED),
        ("the rescale's reserved", dict(rs_reserved=1), UNSUPPORTED),
        ("guidance-only with two operands", dict(plan=make_plan(out0_dtype=_hip.NONE), out=None), UNSUPPORTED),
        ("the draw's samples do not divide the launch", dict(plan=make_plan(sample_numel=4095)), SHAPE),
        ("samples of 4 elements under a draw", dict(plan=make_plan(sample_numel=4), stat_numel=4), UNSUPPORTED),
        ("the statistic's samples of one element", dict(stat_numel=1), SHAPE),
        ("the statistic's samples of no element", dict(stat_numel=0), SHAPE),
        ("the statistic's samples do not divide the launch", dict(plan=make_plan(**quiet), stat_numel=4095), SHAPE),
        ("a drawing plan with another sample", dict(stat_numel=2048), SHAPE),
        ("a plan that does not draw with another sample", dict(plan=make_plan(**quiet), stat_numel=2048, factor=None), NULL),  # (passes the shape check: the next one answers)
        ("empty launch", dict(numel=0, inputs=(None, None), out=None, cond=None, factor=None), OK),
        ("no inputs", dict(no_inputs=True), NULL),
        ("no out", dict(out=None), NULL),
        ("no cond", dict(cond=None), NULL),
        ("no factor", dict(factor=None), NULL),
        ("a NULL operand", dict(inputs=(a, None)), NULL),
        ("a misaligned operand", dict(inputs=(a, b + 2)), ALIGN),
        ("a misaligned guided_out", dict(gout=gout + 8), ALIGN),
        ("a factor aligned to its dtype only", dict(factor=factor + 2, plan=make_plan(out0_dtype=_hip.F16)), DTYPE),  # (no alignment fault: the next check answers)
        ("fp64 operands without acc_f64", dict(plan=make_plan(dtype_a=_hip.F64, out0_dtype=_hip.F64)), DTYPE),
        # two faults: the earlier check answers
        ("no rescale + slot", dict(no_rescale=True, slot=5), NULL),
        ("negative numel + the rescale's reserved", dict(numel=-1, rs_reserved=1), SHAPE),
        ("the rescale's reserved + the draw's sample", dict(rs_reserved=1, plan=make_plan(sample_numel=4095)), UNSUPPORTED),
        ("the draw's sample of 4 + the statistic's of 1", dict(plan=make_plan(sample_numel=4), stat_numel=1), UNSUPPORTED),
        ("the statistic's sample + no factor", dict(stat_numel=1, factor=None), SHAPE),
        ("another sample + no cond", dict(stat_numel=2048, cond=None), SHAPE),
        ("no factor + misaligned out", dict(factor=None, out=out + 4), NULL),
        ("misaligned cond + dtype", dict(cond=cond + 2, plan=make_plan(out0_dtype=_hip.F16)), ALIGN),
    ]
    for what, kwargs, want in table:
        assert call(**kwargs) == want, what
    assert bytes(buf) == bytes(256)  # nothing was written


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.float64])
def test_torch_lines_on_cpu_tensors_are_the_four_diffusers_lines(dtype):
    gen = torch.Generator().manual_seed(5)
    u, c = (torch.randn(3, 4, 8, 8, generator=gen).to(dtype) for _ in range(2))
    g = lazy.Guidance(u, c, 7.3, rescale=0.7)
    assert g.rescale == 0.7 and same_bits(g.torch_lines(), diffusers_lines(u, c, 7.3, 0.7))
    assert same_bits(lazy.guide_only(g), diffusers_lines(u, c, 7.3, 0.7))
    p = u + 7.3 * (c - u)
    want = c.std(dim=[1, 2, 3], keepdim=True) / p.std(dim=[1, 2, 3], keepdim=True)
    assert g.factor().shape == (3, 1, 1, 1) and same_bits(g.factor(), want)
    plain = lazy.Guidance(u, c, 7.3)
    assert plain.rescale == 0.0 and same_bits(plain.torch_lines(), p) and same_bits(lazy.Guidance(u, c, 7.3, rescale=0.0).torch_lines(), p)


def test_rescaled_guidance_is_differentiable_through_torch():
    gen = torch.Generator().manual_seed(6)
    u, c = (torch.randn(2, 4, 8, 8, generator=gen, dtype=torch.float64).requires_grad_() for _ in range(2))
    out = lazy.guide_only(lazy.Guidance(u, c, 5.0, rescale=0.7))
    gu, gc = torch.autograd.grad(out.sum(), (u, c))
    wu, wc = torch.autograd.grad(diffusers_lines(u, c, 5.0, 0.7).sum(), (u, c))
    assert same_bits(gu, wu) and same_bits(gc, wc)


def test_evaluate_guided_on_cpu_tensors_is_the_lines_then_evaluate():
    gen = torch.Generator().manual_seed(3)
    x, u, c = (torch.randn(2, 4, 8, 8, generator=gen).bfloat16() for _ in range(3))
    g = lazy.Guidance(u, c, 7.3, rescale=0.7)
    final, guided = lazy.evaluate_guided(lazy.lift(x) * 1.25 - g.node() * 0.75, g, torch.bfloat16)
    p = diffusers_lines(u, c, 7.3, 0.7)
    assert same_bits(guided, p)
    assert same_bits(final, lazy.evaluate([lazy.lift(x) * 1.25 - lazy.lift(p) * 0.75], [torch.bfloat16])[0])


SAMPLERS = {"euler": lambda: PT.Euler(), "dpm2": lambda: PT.DPM(order=2), "unipc2": lambda: PT.UniPC(order=2)}


@pytest.mark.parametrize("name", sorted(SAMPLERS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_guided_with_rescale_on_cpu_tensors_equals_step_of_the_lines_bit_for_bit(name, dtype):
    shape, steps, scale, phi = (2, 4, 8, 8), 6, 7.3, 0.7
    make = lambda: PD.SkrampleWrapperScheduler(SAMPLERS[name](), PS.Karras(PS.Scaled()))  # noqa: E731
    fused, plain = make(), make()
    fused.set_timesteps(steps), plain.set_timesteps(steps)
    g = torch.Generator().manual_seed(11)
    xa = xb = torch.randn(shape, generator=g).to(dtype)
    for i, t in enumerate(list(plain.timesteps)):
        both = torch.randn((4, *shape[1:]), generator=g).to(dtype)
        uncond, cond = both.chunk(2)
        if i % 3 == 2:  # a run may mix rescaled calls with plain guided ones
            xa, pa = fused.step_guided(uncond, cond, scale, t, xa, return_dict=False)
            xb, pb = plain.step(uncond + scale * (cond - uncond), t, xb, return_dict=False)
        else:
            xa, pa = fused.step_guided(uncond, cond, scale, t, xa, return_dict=False, guidance_rescale=phi)
            xb, pb = plain.step(diffusers_lines(uncond, cond, scale, phi), t, xb, return_dict=False)
        assert same_bits(xa, xb) and same_bits(pa, pb), i


def test_guidance_rescale_zero_is_the_call_without_the_keyword():
    "on the host no launch is traced either way; the results are identical, and the keyword is the last one"
    import inspect

    assert list(inspect.signature(PD.SkrampleWrapperScheduler.step_guided).parameters)[-1] == "guidance_rescale"
    assert list(inspect.signature(graphs.capture_sampling_loop).parameters)[-1] == "guidance_rescale"
    from skrample_amd import rolling

    assert "guidance_rescale" not in inspect.signature(rolling.RollingBatch.step_guided).parameters and "guidance_rescale" not in inspect.signature(rolling.RollingBatch.__init__).parameters
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))  # noqa: E731
    with_kw, without = make(), make()
    with_kw.set_timesteps(4), without.set_timesteps(4)
    g = torch.Generator().manual_seed(2)
    x, u, c = (torch.randn(2, 4, 8, 8, generator=g) for _ in range(3))
    traces = []
    for w, kw in ((with_kw, dict(guidance_rescale=0.0)), (without, {})):
        _hip.trace = []
        try:
            traces.append((w.step_guided(u, c, 5.0, w.timesteps[0], x, return_dict=False, **kw), list(_hip.trace)))
        finally:
            _hip.trace = None
    (ra, ta), (rb, tb) = traces
    assert ta == tb == [] and same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


def test_refusals_say_why():
    u = torch.randn(2, 4, 8, 8)
    with pytest.raises(lazy.SkrampleHipError, match="guidance_rescale must be >= 0"):
        lazy.Guidance(u, u.clone(), 7.5, rescale=-0.1)
    with pytest.raises(lazy.SkrampleHipError, match="guidance_rescale must be >= 0"):
        lazy.Guidance(u, u.clone(), 7.5, rescale=float("nan"))
    for bad in ("0.7", torch.tensor(0.7), True, None):
        with pytest.raises(lazy.SkrampleHipError, match="guidance_rescale is a Python number"):
            lazy.Guidance(u, u.clone(), 7.5, rescale=bad)
    flat = torch.randn(64)
    with pytest.raises(lazy.SkrampleHipError, match="ndim >= 2"):
        lazy.Guidance(flat, flat.clone(), 7.5, rescale=0.7)
    with pytest.raises(lazy.SkrampleHipError, match="ndim >= 2"):
        lazy.Guidance(flat, flat.clone(), 7.5).factor()
    assert lazy.Guidance(flat, flat.clone(), 7.5).rescale == 0.0  # (without rescale a flat tensor is guided as ever)
    w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled()))
    w.set_timesteps(4)
    with pytest.raises(lazy.SkrampleHipError, match="guidance_rescale must be >= 0"):
        w.step_guided(u, u.clone(), 7.5, w.timesteps[0], u.clone(), guidance_rescale=-1.0)
    with pytest.raises(ValueError, match="guidance_scale"):
        graphs.capture_sampling_loop(w, lambda x, t: (x, x), u, 4, guidance_rescale=0.7)
    # a captured loop with device-resident rows: both launches refuse by name while the rows hook is installed (its recording pass)
    _hip.indexed = object()
    try:
        with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale.*no row form"):
            _hip.launch_guidance_factor(u, u, 7.5, 256, u)
        with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale.*no row form"):
            _hip.launch_step_guided_rescaled(_hip.StepPlanC(), [u], None, u, u, 7.5, 0, u, 0.7, 256, None, 512, u.device)
    finally:
        _hip.indexed = None
