"""Channels-last steps without a device: the two C ABI entries are declared in the header, listed by the binding and exported by the
built library; the ABI version has not moved; the header is still plain C; the layout checks of every entry that takes a layout answer
before any pointer is dereferenced; and lazy.layout_of tells a dense channels-last tensor from everything else."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from skrample_amd import _hip
from skrample_amd.sampling import lazy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("skr_step_launch_channels_last", "skr_program_create_channels_last")
OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED = 0, 1, 5, 7


def test_header_binding_and_library_have_the_two_entries():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    ws = r"\s*"
    launch = (r"const\s+skr_step_plan\s*\*\s*plan", r"const\s+void\s*\*\s*const\s*\*\s*inputs", r"void\s*\*\s*out0", r"void\s*\*\s*out1",
              r"const\s+uint64_t\s*\*\s*seeds_dev", r"const\s+skr_step_layout\s*\*\s*layout", r"int64_t\s+numel", r"void\s*\*\s*stream")  # fmt: skip
    create = (r"const\s+skr_step_plan\s*\*\s*plan", r"int64_t\s+numel", r"const\s+skr_step_layout\s*\*\s*layout", r"skr_program\s*\*\s*\*\s*out")
    for name, args in zip(NAMES, (launch, create)):
        assert re.search(rf"^int\s+{name}{ws}\({ws}" + rf"{ws},{ws}".join(args) + rf"{ws}\){ws};", flat, flags=re.M), name
        assert name in _hip.EXPORTS
    assert re.search(r"typedef\s+struct\s+skr_step_layout\s*\{\s*int64_t\s+channels\s*;\s*int64_t\s+plane\s*;\s*\}\s*skr_step_layout\s*;", flat)
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15  # purely additive
    lib = _hip.load()
    assert lib.skr_abi_version() == 15
    assert len(lib.skr_step_launch_channels_last.argtypes) == 8 and lib.skr_step_launch_channels_last.restype is ctypes.c_int
    assert len(lib.skr_program_create_channels_last.argtypes) == 4 and lib.skr_program_create_channels_last.restype is ctypes.c_int
    assert ctypes.sizeof(_hip.StepLayoutC) == 16


def test_header_is_still_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
        "int main(void) {\n"
        "  skr_step_layout layout = {4, 1024};\n"
        "  int (*launch)(const skr_step_plan*, const void* const*, void*, void*, const uint64_t*, const skr_step_layout*, int64_t, void*) = skr_step_launch_channels_last;\n"
        "  int (*create)(const skr_step_plan*, int64_t, const skr_step_layout*, skr_program**) = skr_program_create_channels_last;\n"
        "  (void)layout; (void)launch; (void)create;\n"
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
    plan.sample_numel = sample_numel
    plan.noise_mode, plan.zeta0, plan.stream0 = 1, 0.5, 256
    for key, value in fields.items():
        setattr(plan, key, value)
    return plan


def test_layout_checks_answer_before_any_pointer_is_dereferenced():
    """host buffers that are never read stand in for device pointers: every status below is returned ahead of the launch.  The three
    entries that take a layout -- the plain launch, the program made for it, the masked launch -- answer the same bad layouts alike"""
    lib = _hip.load()
    blob = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(blob) + 15) & ~15  # 16-byte aligned stand-ins (the alignment check of skr_step_launch comes first)
    arr = (ctypes.c_void_p * 2)(base, base + 64)
    out, seeds, numel = base + 128, base + 256, 2 * 4096
    handle = ctypes.c_void_p()
    mask = _hip.StepMaskC(base + 512, _hip.BF16, 0, 1024, 1024)

    def ref(layout):
        return ctypes.byref(layout) if layout is not None else None

    def launch(plan, layout, out1=None):
        return lib.skr_step_launch_channels_last(ctypes.byref(plan), arr, out, out1, seeds, ref(layout), numel, None)

    def create(plan, layout, out1=None):
        status = lib.skr_program_create_channels_last(ctypes.byref(plan), numel, ref(layout), ctypes.byref(handle))
        assert bool(handle.value) == (status == OK)
        return status

    def masked(plan, layout, out1=None):
        plan.coef1[1] = 0.25
        return lib.skr_step_launch_masked_channels_last(ctypes.byref(plan), arr, out, ctypes.byref(mask), seeds, ref(layout), numel, None)

    convert = dict(out1_dtype=_hip.BF16, convert_to=1, convert_from=1)
    for entry in (launch, create, masked):
        assert entry(make_plan(), None) == ERR_NULL, entry.__name__
        for channels, plane in ((4, 1000), (0, 4096), (4, 0), (-4, -1024), (3, 1024)):  # channels * plane != sample_numel, channels < 1, plane < 1
            assert entry(make_plan(), _hip.StepLayoutC(channels, plane)) == ERR_SHAPE, (entry.__name__, channels, plane)
        assert entry(make_plan(sample_numel=4096, noise_mode=0, zeta0=0.0), _hip.StepLayoutC(4, 1000)) == ERR_SHAPE  # (with or without a draw)
        if entry is not masked:  # a draw together with a rounded conversion (a masked launch has no conversion)
            assert entry(make_plan(**convert), _hip.StepLayoutC(4, 1024), out1=base + 512) == ERR_UNSUPPORTED, entry.__name__
    # skr_step_launch's own checks keep their place in front: a NULL plan, a missing seed pointer, a sample size that does not divide
    assert lib.skr_step_launch_channels_last(None, arr, out, None, seeds, ctypes.byref(_hip.StepLayoutC(4, 1024)), numel, None) == ERR_NULL
    assert lib.skr_step_launch_channels_last(ctypes.byref(make_plan()), arr, out, None, None, None, numel, None) == ERR_NULL
    assert launch(make_plan(sample_numel=4095), _hip.StepLayoutC(4, 1024)) == ERR_SHAPE
    # programs: a good layout makes a handle
    assert create(make_plan(), _hip.StepLayoutC(4, 1024)) == OK and handle.value
    lib.skr_program_destroy(handle.value)


def test_layout_of_tells_dense_channels_last_from_everything_else():
    x = torch.zeros(2, 4, 8, 8)
    assert lazy.layout_of(x.to(memory_format=torch.channels_last)) == (4, 64)
    assert lazy.layout_of(torch.zeros(2, 4, 2, 8, 8).to(memory_format=torch.channels_last_3d)) == (4, 128)
    assert lazy.layout_of(torch.zeros(1, 4, 8, 8).to(memory_format=torch.channels_last)) == (4, 64)  # (a batch of one: its stride is free)
    assert lazy.layout_of(x) is None  # contiguous
    assert lazy.layout_of(torch.zeros(2, 1, 8, 8).to(memory_format=torch.channels_last)) is None  # C = 1: storage order = logical order
    assert lazy.layout_of(torch.zeros(2, 4, 8, 16).to(memory_format=torch.channels_last)[..., ::2]) is None  # not dense
    assert lazy.layout_of(x.permute(0, 2, 1, 3)) is None  # another permutation
    assert lazy.layout_of(torch.zeros(8, 4).t()) is None  # rank 2
    assert lazy.layout_of(torch.zeros(2, 4, 1, 1).to(memory_format=torch.channels_last)) is None  # a plane of one position
    assert lazy.channels_last is True
    cl = x.to(memory_format=torch.channels_last)
    assert lazy.shared_layout([cl, cl.clone()], cl.shape) == (4, 64)
    assert lazy.shared_layout([cl, x], cl.shape) is None  # mixed layouts: today's path
