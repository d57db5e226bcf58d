"""The row forms of dynamic thresholding without a device: the four entries in the header and in the binding, the ABI and the launch table
untouched, the header as C99, and the checks the entries make before anything is launched."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest

from skrample_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "skrample_hip.h")
NAMES = ["skr_threshold_scale_indexed", "skr_threshold_scale_indexed_per_sample", "skr_thresholded_step_launch_indexed", "skr_thresholded_step_launch_indexed_per_sample"]
OK, NULL, DTYPE, TERMS, ALIGN, SHAPE, LAUNCH, UNSUPPORTED = range(8)


def test_entries_are_declared_and_additive():
    text = open(HEADER).read()
    for name in NAMES:
        assert re.search(rf"^int {name}\(", text, re.M) and name in _hip.EXPORTS, name
    assert _hip.ABI_VERSION == 15 and "#define SKR_ABI_VERSION 15" in text
    assert len(_hip.ENTRIES) == 22 and not any(name in NAMES for name, _ in _hip.ENTRIES.values())  # outside the launch table, as the direct two are


def test_header_compiles_as_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "rows.c"
    uses = "".join(f"  (void){name};\n" for name in NAMES)
    src.write_text(f'#include "{HEADER}"\nint main(void) {{\n{uses}  return 0;\n}}\n')
    done = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "rows.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


@pytest.mark.parametrize("per_sample", [False, True], ids=["indexed", "per_sample"])
def test_checks_in_their_documented_order(per_sample):
    lib = _hip.load()
    buf = (ctypes.c_char * 128)()
    good = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    suffix = "_indexed_per_sample" if per_sample else "_indexed"

    def scale(sample=good, dtype=_hip.BF16, numel=4096, sn=2048, rows=good, index=good, offset=0, out=good, ws=good):
        return getattr(lib, "skr_threshold_scale" + suffix)(sample, good, dtype, numel, sn, rows, index, offset, out, ws, None)

    assert scale(sample=None, numel=-1) == NULL and scale(rows=None, sn=0) == NULL and scale(index=None, sn=0) == (NULL if per_sample else SHAPE)
    assert scale(numel=-8) == SHAPE and scale(sn=0) == SHAPE and scale(numel=4097) == SHAPE
    assert scale(numel=0, sample=good + 8, dtype=99, offset=-1) == OK  # an empty launch ahead of everything behind it
    assert scale(sample=good + 8, dtype=99) == ALIGN and scale(out=good + 2, dtype=99) == ALIGN
    assert scale(dtype=_hip.F64, sn=8, numel=16) == DTYPE
    assert scale(sn=8, numel=16) == UNSUPPORTED and scale(offset=-1) == UNSUPPORTED  # no ragged form, no negative offset

    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 2
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    ops = (ctypes.c_void_p * 2)(good, good)

    def step(numel=2048, out=good, rows=good, index=good, offset=0, scale_dev=good, sn=2048, **changes):
        thr = _hip.StepThresholdC(scale_dev, good, 0.0, 0.0, sn, 0, 1, 0)
        saved = {k: getattr(plan, k) for k in changes}
        for k, v in changes.items():
            setattr(plan, k, v)
        status = getattr(lib, "skr_thresholded_step_launch" + suffix)(ctypes.byref(plan), ops, out, ctypes.byref(thr), None, numel, rows, index, offset, None)
        for k, v in saved.items():
            setattr(plan, k, v)
        return status

    assert step(rows=None, n_terms=99) == NULL and step(index=None, n_terms=99) == (NULL if per_sample else TERMS)
    assert step(noise_mode=1, n_terms=99) == NULL  # a plan that may draw without seeds (the row's zeta decides, so zeta0 == 0 does not excuse it)
    assert step(n_terms=17, numel=-1) == TERMS and step(numel=-1, noise_mode=3) == SHAPE
    assert step(convert_to=1, sn=0) == UNSUPPORTED and step(acc_f64=1, sn=0) == UNSUPPORTED and step(sn=0) == SHAPE
    assert step(chain=1.0, zeta1=1.0, numel=0) == OK  # the plan's scalars are not read
    assert step(scale_dev=None) == NULL and step(out=good + 8) == ALIGN and step(scale_dev=good + 2) == ALIGN
    assert step(dtype_a=99) == DTYPE
    assert step(numel=16, sn=8) == UNSUPPORTED and step(offset=-1) == UNSUPPORTED and step(dtype_b=_hip.F32, n_group_a=1) == UNSUPPORTED
