"""Guided steps (classifier-free guidance) without a device: the C ABI declaration, its binding and its checks, lazy.Guidance, and
SkrampleWrapperScheduler.step_guided on CPU tensors.

The contract is one sentence -- a guided step returns the bits of the pipeline's three torch lines followed by step() -- so every
comparison here is made on the integer views of the bits.  Host-resident operands evaluate the three lines with torch itself and then
the existing host executor: equality is by construction, and what is tested is that the wrapper's bookkeeping (history, the aliasing
guard, mixed runs, invert_prediction) stays that of step()."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "skr_step_launch_guided"
FIELDS = ["cond", "guided_out", "scale", "slot", "reserved"]
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def same_bits(a, b):
    a, b = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (a, b))  # (pred_original_sample may be lazy)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype]))


def test_header_declares_the_entry_and_the_binding_lists_it():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"int\s+skr_step_launch_guided\s*\(\s*const\s+skr_step_plan\s*\*\s*plan,\s*const\s+void\s*\*\s*const\s*\*\s*inputs,\s*void\s*\*\s*out,\s*const\s+skr_step_guidance\s*\*", header)
    body = re.search(r"typedef\s+struct\s+skr_step_guidance\s*\{(.*?)\}\s*skr_step_guidance\s*;", header, re.S)
    assert body is not None
    assert re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)) == FIELDS
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15
    assert NAME in _hip.EXPORTS and callable(_hip.launch_step_guided)


def test_the_built_library_exports_the_entry():
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    entry = getattr(lib, NAME)
    assert len(entry.argtypes) == 7 and entry.restype is ctypes.c_int


def test_binding_struct_has_the_size_and_offsets_of_the_c_struct(tmp_path):
    assert [name for name, _ in _hip.StepGuidanceC._fields_] == FIELDS
    want = {"cond": 0, "guided_out": 8, "scale": 16, "slot": 24, "reserved": 28}
    assert {name: getattr(_hip.StepGuidanceC, name).offset for name in FIELDS} == want and ctypes.sizeof(_hip.StepGuidanceC) == 32
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    # the compiler's own answer: one _Static_assert per figure
    src = tmp_path / "layout.c"
    checks = "".join(f'_Static_assert(offsetof(skr_step_guidance, {name}) == {off}, "{name}");\n' for name, off in want.items())
    src.write_text(f'#include <stddef.h>\n#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n{checks}_Static_assert(sizeof(skr_step_guidance) == 32, "size");\nint main(void) {{ return 0; }}\n')
    done = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "layout.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_header_is_still_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        "int main(void) {\n"
        "  skr_step_guidance guide = {0, 0, 7.5, 1, 0};\n"
        "  int (*launch)(const skr_step_plan*, const void* const*, void*, const skr_step_guidance*, const uint64_t*, int64_t, void*) =\n"
        f"      {NAME};\n"
        "  (void)guide; (void)launch;\n"
        f"  return SKR_ABI_VERSION == {_hip.ABI_VERSION} ? 0 : 1;\n"
        "}\n"
    )
    done = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "client.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


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


def test_checks_answer_before_any_pointer_is_dereferenced_and_in_order():
    "host buffers that are never read stand in for device pointers: every status below is returned ahead of the launch"
    lib = _hip.load()
    entry = getattr(lib, NAME)
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, out, cond, gout, seeds = (base + 32 * k for k in range(6))
    numel = 8192

    def call(plan=None, inputs=(a, b), out=out, cond=cond, gout=gout, scale=7.5, slot=1, reserved=0, seeds=seeds, numel=numel, no_plan=False, no_guide=False, no_inputs=False):
        plan = plan if plan is not None else make_plan()
        arr = (ctypes.c_void_p * max(len(inputs), 1))(*inputs)
        guide = _hip.StepGuidanceC(cond, gout, scale, slot, reserved)
        return entry(None if no_plan else ctypes.byref(plan), None if no_inputs else arr, out, None if no_guide else ctypes.byref(guide), seeds, numel, None)

    table = [
        ("no plan", dict(no_plan=True), NULL),
        ("no guide", dict(no_guide=True), NULL),
        ("a draw without seeds", dict(seeds=None), NULL),
        ("too many operands", dict(plan=make_plan(n_terms=17, n_group_a=17)), TERMS),
        ("group a beyond the operands", dict(plan=make_plan(n_group_a=3)), TERMS),
        ("slot below the operands", dict(slot=-1), TERMS),
        ("slot beyond the operands", dict(slot=2), TERMS),
        ("negative numel", dict(numel=-8), SHAPE),
        ("no output at all", dict(plan=make_plan(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1, noise_mode=0), inputs=(a,), out=None, gout=None, slot=0), NULL),
        ("noise_mode 2", dict(plan=make_plan(noise_mode=2)), UNSUPPORTED),
        ("a second output", dict(plan=make_plan(out1_dtype=_hip.BF16)), UNSUPPORTED),
        ("chain", dict(plan=make_plan(chain=0.5)), UNSUPPORTED),
        ("zeta1", dict(plan=make_plan(zeta1=0.5)), UNSUPPORTED),
        ("convert_to", dict(plan=make_plan(convert_to=1)), UNSUPPORTED),
        ("convert_from", dict(plan=make_plan(convert_from=4)), UNSUPPORTED),
        ("reserved", dict(reserved=1), UNSUPPORTED),
        ("guidance-only with two operands", dict(plan=make_plan(out0_dtype=_hip.NONE), out=None), UNSUPPORTED),
        ("guidance-only with an out pointer", dict(plan=make_plan(out0_dtype=_hip.NONE, n_terms=1, n_group_a=1), inputs=(a,), slot=0), UNSUPPORTED),
        ("samples that do not divide the launch", dict(plan=make_plan(sample_numel=4095)), SHAPE),
        ("no sample size under a draw", dict(plan=make_plan(sample_numel=0)), SHAPE),
        ("samples of 4 elements under a draw", dict(plan=make_plan(sample_numel=4)), UNSUPPORTED),
        ("empty launch", dict(numel=0, inputs=(None, None), out=None, cond=None), OK),
        ("no inputs", dict(no_inputs=True), NULL),
        ("no out", dict(out=None), NULL),
        ("no cond", dict(cond=None), NULL),
        ("a NULL operand", dict(inputs=(a, None)), NULL),
        ("a misaligned operand", dict(inputs=(a, b + 2)), ALIGN),
        ("a misaligned out", dict(out=out + 4), ALIGN),
        ("a misaligned cond", dict(cond=cond + 2), ALIGN),
        ("a misaligned guided_out", dict(gout=gout + 8), ALIGN),
        ("fp64 operands without acc_f64", dict(plan=make_plan(dtype_a=_hip.F64, out0_dtype=_hip.F64)), DTYPE),
        ("an fp64 group b without acc_f64", dict(plan=make_plan(n_group_a=1, dtype_b=_hip.F64)), DTYPE),
        ("an out dtype outside the groups", dict(plan=make_plan(out0_dtype=_hip.F16)), DTYPE),
        ("a dtype code that names none", dict(plan=make_plan(dtype_a=9, out0_dtype=9)), DTYPE),
        # two faults: the earlier check answers
        ("no seeds + slot", dict(seeds=None, slot=5), NULL),
        ("slot + negative numel", dict(slot=2, numel=-1), TERMS),
        ("negative numel + reserved", dict(numel=-1, reserved=1), SHAPE),
        ("reserved + sample size", dict(reserved=1, plan=make_plan(sample_numel=4095)), UNSUPPORTED),
        ("sample size + no cond", dict(plan=make_plan(sample_numel=4095), cond=None), SHAPE),
        ("no cond + misaligned out", dict(cond=None, out=out + 4), NULL),
        ("misaligned cond + dtype", dict(cond=cond + 2, plan=make_plan(out0_dtype=_hip.F16)), ALIGN),
    ]
    for what, kwargs, want in table:
        assert call(**kwargs) == want, what
    assert bytes(buf) == bytes(256)  # nothing was written


def test_guidance_refuses_what_it_does_not_take():
    u = torch.randn(2, 4, 8, 8)
    for bad in [(u, u.double(), 7.5), (u, torch.randn(2, 4, 8, 4), 7.5), (u, u.to("meta"), 7.5), (u, [1.0], 7.5), (3.0, u, 7.5), (u, u, torch.tensor(7.5)), (u, u, "7.5"), (u, u, True)]:
        with pytest.raises((lazy.SkrampleHipError, TypeError)):
            lazy.Guidance(*bad)
    g = lazy.Guidance(u, u.clone(), 3)
    assert g.scale == 3.0 and g.dtype == torch.float32 and g.shape == (2, 4, 8, 8)
    node = g.node()
    assert isinstance(node, lazy.Lin) and len(node.terms) == 1 and isinstance(next(iter(node.terms.values()))[0], lazy.Node)
    with pytest.raises(lazy.SkrampleHipError):  # not a linear form: only evaluate_guided settles it
        lazy.evaluate([node], [None])


def test_evaluate_guided_on_cpu_tensors_is_the_three_lines_then_evaluate():
    gen = torch.Generator().manual_seed(3)
    x, u, c = (torch.randn(2, 4, 8, 8, generator=gen).bfloat16() for _ in range(3))
    g = lazy.Guidance(u, c, 7.3)
    final, guided = lazy.evaluate_guided(lazy.lift(x) * 1.25 - g.node() * 0.75, g, torch.bfloat16)
    p = u + 7.3 * (c - u)
    assert same_bits(guided, p)
    assert same_bits(final, lazy.evaluate([lazy.lift(x) * 1.25 - lazy.lift(p) * 0.75], [torch.bfloat16])[0])


SAMPLERS = {"euler": lambda: PT.Euler(), "dpm2": lambda: PT.DPM(order=2), "unipc2": lambda: PT.UniPC(order=2)}


@pytest.mark.parametrize("name", sorted(SAMPLERS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("invert", [False, True])
def test_step_guided_on_cpu_tensors_equals_the_unfused_run_bit_for_bit(name, dtype, invert):
    shape, steps, scale = (2, 4, 8, 8), 6, 7.3
    make = lambda: PD.SkrampleWrapperScheduler(SAMPLERS[name](), PS.Karras(PS.Scaled()), invert_prediction=invert)  # noqa: E731
    fused, plain = make(), make()
    fused.set_timesteps(steps), plain.set_timesteps(steps)
    g = torch.Generator().manual_seed(11)
    xa = xb = torch.randn(shape, generator=g).to(dtype)
    for i, t in enumerate(list(plain.timesteps)):
        both = torch.randn((4, *shape[1:]), generator=g).to(dtype)
        uncond, cond = both.chunk(2)
        if i % 2:  # a run may mix the two calls
            xa, pa = fused.step_guided(uncond, cond, scale, t, xa, return_dict=False)
        else:
            xa, pa = fused.step(uncond + scale * (cond - uncond), t, xa, return_dict=False)
        xb, pb = plain.step(uncond + scale * (cond - uncond), t, xb, return_dict=False)
        assert same_bits(xa, xb) and same_bits(pa, pb), i


def test_step_guided_returns_what_step_returns_and_the_rk_wrappers_have_none():
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    w.set_timesteps(4)
    x, u, c = torch.randn(2, 4, 8, 8), torch.randn(2, 4, 8, 8), torch.randn(2, 4, 8, 8)
    out = w.step_guided(u, c, 5.0, w.timesteps[0], x)
    assert set(out.keys()) == {"prev_sample", "pred_original_sample"} and out.prev_sample.dtype == x.dtype
    assert not w._programs and not w._fast  # no step program, no replayed entry
    assert not hasattr(PD.RKUltraWrapperScheduler, "step_guided") and not hasattr(PD.DynasauRKWrapperScheduler, "step_guided")
    with pytest.raises(lazy.SkrampleHipError):
        w.step_guided(u, c.double(), 5.0, w.timesteps[1], x)
