"""Masked channels-last steps without a device: skr_step_launch_masked_channels_last is declared in the header, listed by the binding
and exported by the built library; the ABI version has not moved; the header is still plain C; and the entry's checks answer before any
pointer is dereferenced, in their order: skr_step_launch_masked's own, then the layout pointer, then the layout's shape, then an empty
launch."""

import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

from skrample_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "skr_step_launch_masked_channels_last"
OK, ERR_NULL, ERR_DTYPE, ERR_TERMS, ERR_ALIGN, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5, 7


def test_header_binding_and_library_have_the_entry():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    args = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out", r"const\s+skr_step_mask\s*\*\s*mask",
            r"const\s+uint64_t\s*\*\s*seeds_dev", r"const\s+skr_step_layout\s*\*\s*layout", r"int64_t\s+numel", r"void\s*\*\s*stream")  # fmt: skip
    assert re.search(rf"^int\s+{NAME}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M)
    assert NAME in _hip.EXPORTS and "layout" in inspect.signature(_hip.launch_step_masked).parameters
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    entry = getattr(lib, NAME)
    assert len(entry.argtypes) == 8 and entry.restype is ctypes.c_int
    for key in (b"masked_channels_last_one_trip", b"masked_channels_last_general"):
        assert lib.skr_stat(key) >= 0, key
    assert lib.skr_stat(b"masked_channels_last") == -1


def test_header_is_still_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        "int main(void) {\n"
        "  skr_step_layout layout = {4, 1024};\n"
        "  int (*launch)(const skr_step_plan*, const void* const*, void*, const skr_step_mask*, const uint64_t*, const skr_step_layout*, int64_t, void*) =\n"
        f"      {NAME};\n"
        "  (void)layout; (void)launch;\n"
        f"  return SKR_ABI_VERSION == {_hip.ABI_VERSION} ? 0 : 1;\n"
        "}\n"
    )
    done = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "client.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def make_plan(sample_numel=4096, **fields):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.out0_dtype = _hip.BF16
    plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
    plan.coef0[0], plan.coef0[1] = 1.0, -0.5
    plan.coef1[1] = 0.25
    plan.sample_numel = sample_numel
    plan.noise_mode, plan.zeta0, plan.stream0 = 1, 0.5, 256
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def test_checks_answer_before_any_pointer_is_dereferenced_and_in_order():
    "host buffers that are never read stand in for device pointers: every status below is returned ahead of the launch"
    lib = _hip.load()
    entry = getattr(lib, NAME)
    blob = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(blob) + 15) & ~15  # 16-byte aligned stand-ins
    arr = (ctypes.c_void_p * 2)(base, base + 64)
    out, seeds, numel = base + 128, base + 256, 2 * 4096
    good = _hip.StepLayoutC(4, 1024)

    def mask_desc(ptr=base + 512, dtype=_hip.BF16, reserved=0, mask_numel=1024, batch_stride=1024):
        return _hip.StepMaskC(ptr, dtype, reserved, mask_numel, batch_stride)

    def launch(plan, layout, mask=None, n=numel, out_ptr=out, seeds_ptr=seeds, inputs=arr):
        mask = mask if mask is not None else mask_desc()
        return entry(ctypes.byref(plan), inputs, out_ptr, ctypes.byref(mask), seeds_ptr, ctypes.byref(layout) if layout is not None else None, n, None)

    # the layout's own checks
    assert launch(make_plan(), None) == ERR_NULL
    for channels, plane in ((4, 1000), (0, 4096), (4, 0), (-4, -1024), (3, 1024), (8, 1024)):
        assert launch(make_plan(), _hip.StepLayoutC(channels, plane)) == ERR_SHAPE, (channels, plane)
    assert launch(make_plan(noise_mode=0, zeta0=0.0), _hip.StepLayoutC(4, 1000)) == ERR_SHAPE  # (with or without a draw)
    # an empty launch: SKR_OK behind the layout's checks, pointers never looked at
    assert launch(make_plan(), good, n=0, out_ptr=None, seeds_ptr=None, inputs=None) == OK
    assert launch(make_plan(), None, n=0) == ERR_NULL
    assert launch(make_plan(), _hip.StepLayoutC(4, 1000), n=0) == ERR_SHAPE
    # skr_step_launch_masked's own checks keep their place in front of the layout's: each of these meets a NULL or a wrong layout too
    for layout in (None, _hip.StepLayoutC(4, 1000)):
        assert entry(None, arr, out, ctypes.byref(mask_desc()), seeds, ctypes.byref(good), numel, None) == ERR_NULL
        assert entry(ctypes.byref(make_plan()), arr, out, None, seeds, ctypes.byref(good), numel, None) == ERR_NULL
        assert launch(make_plan(n_terms=17, n_group_a=17), layout) == ERR_TERMS
        assert launch(make_plan(n_group_a=3), layout) == ERR_TERMS
        assert launch(make_plan(), layout, n=-1) == ERR_SHAPE
        assert launch(make_plan(out0_dtype=_hip.NONE), layout) == ERR_NULL
        assert launch(make_plan(out1_dtype=_hip.BF16), layout) == ERR_UNSUPPORTED
        assert launch(make_plan(chain=0.5), layout) == ERR_UNSUPPORTED
        assert launch(make_plan(), layout, mask=mask_desc(reserved=1)) == ERR_UNSUPPORTED
        assert launch(make_plan(sample_numel=4095), layout) == ERR_SHAPE
        assert launch(make_plan(), layout, mask=mask_desc(mask_numel=1000)) == ERR_SHAPE
        assert launch(make_plan(), layout, mask=mask_desc(batch_stride=512)) == ERR_SHAPE
        assert launch(make_plan(dtype_a=_hip.F64), layout) == ERR_DTYPE
        assert launch(make_plan(), layout, mask=mask_desc(dtype=_hip.F64)) == ERR_DTYPE
        assert launch(make_plan(), layout, seeds_ptr=None) == ERR_NULL  # a draw without seeds
        assert launch(make_plan(), layout, mask=mask_desc(ptr=None)) == ERR_NULL
        assert launch(make_plan(), layout, out_ptr=out + 2) == ERR_ALIGN
        assert launch(make_plan(), layout, mask=mask_desc(ptr=base + 514)) == ERR_ALIGN
    # and with a good layout they are what skr_step_launch_masked itself answers
    plain = lib.skr_step_launch_masked
    for plan, mask in ((make_plan(sample_numel=4095), mask_desc()), (make_plan(), mask_desc(mask_numel=1000)), (make_plan(chain=0.5), mask_desc())):
        want = plain(ctypes.byref(plan), arr, out, ctypes.byref(mask), seeds, numel, None)
        assert want != OK and launch(plan, good, mask=mask) == want
