"""The masked backward launch without a device: skr_step_masked_backward_launch is declared in the header, listed by the binding and
exported by the built library; the ABI version has not moved; the header is still plain C; and lazy.evaluate_masked keeps refusing what it
has no gradient for -- host-resident operands that require grad (the host executor of a masked step has no backward) and a mask that
requires grad (it would need the operands and a reduction over the broadcast axes)."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
from conftest import ROOT

from skrample_amd import _hip
from skrample_amd.sampling import lazy

HEADER = os.path.join(ROOT, "include", "skrample_hip.h")
NAME = "skr_step_masked_backward_launch"


def test_the_entry_is_declared_listed_and_exported():
    header = open(HEADER).read()
    assert re.search(
        rf"int\s+{NAME}\s*\(\s*const\s+skr_step_grad_plan\s*\*\s*plan,\s*const\s+void\s*\*\s*g,\s*const\s+skr_step_mask\s*\*\s*mask,\s*"
        r"void\s*\*\s*const\s*\*\s*grads,\s*int64_t\s+numel,\s*int64_t\s+sample_numel,\s*void\s*\*\s*stream\s*\)", header)  # fmt: skip
    assert NAME in _hip.EXPORTS
    assert os.path.isfile(_hip.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), NAME)
    entry = getattr(_hip.load(), NAME)
    assert entry.restype is ctypes.c_int and len(entry.argtypes) == 7
    assert callable(lazy.launch_masked_backward) and issubclass(lazy._MaskedStepFunction, torch.autograd.Function)


def test_the_abi_version_is_still_15():
    header = open(HEADER).read()
    assert re.search(r"#define\s+SKR_ABI_VERSION\s+15\b", header) and _hip.ABI_VERSION == 15
    assert _hip.load().skr_abi_version() == 15


def test_argument_checks_that_need_no_device():
    "refused before anything is launched: no pointer here is device memory"
    lib = _hip.load()
    plan, mask = _hip.StepGradPlanC(), _hip.StepMaskC(None, _hip.F32, 0, 8, 8)
    plan.n_grads = plan.n_group_a = 1
    plan.dtype_a = plan.dtype_b = plan.g0_dtype = _hip.F32
    plan.g1_dtype = _hip.NONE
    arr = (ctypes.c_void_p * 1)(None)
    call = lambda p=plan, m=mask, grads=arr, numel=16: getattr(lib, NAME)(ctypes.byref(p) if p is not None else None, None, ctypes.byref(m) if m is not None else None, grads, numel, 16, None)  # noqa: E731
    assert call(p=None) == 1 and call(m=None) == 1 and call(grads=None) == 1  # SKR_ERR_NULL
    assert call() == 1  # g is NULL
    assert call(numel=0) == 0  # an empty batch: nothing to do
    assert call(numel=-1) == 5 and call(numel=24) == 5  # SKR_ERR_SHAPE
    plan.n_grads = plan.n_group_a = _hip.ROW_TERMS + 1
    assert call() == 3  # SKR_ERR_TERMS
    plan.n_grads = plan.n_group_a = 1
    plan.g1_dtype = _hip.F32
    assert call() == 7  # SKR_ERR_UNSUPPORTED: one incoming gradient only


def test_the_header_is_still_plain_c(tmp_path):
    "a C99 client that names the new entry and the two structures it reuses compiles without a warning"
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "client.c"
    src.write_text(
        f'#include "{HEADER}"\n'
        "int main(void) {\n"
        "  skr_step_grad_plan plan; skr_step_mask mask;\n"
        "  int (*entry)(const skr_step_grad_plan*, const void*, const skr_step_mask*, void* const*, int64_t, int64_t, void*) = skr_step_masked_backward_launch;\n"
        "  (void)plan; (void)mask; (void)entry;\n"
        f"  return SKR_ABI_VERSION == {_hip.ABI_VERSION} && SKR_ROW_TERMS == {_hip.ROW_TERMS} ? 0 : 1;\n"
        "}\n"
    )
    done = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "client.o")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def _forms(requires_grad: bool):
    g = torch.Generator().manual_seed(3)
    x, orig = torch.randn(2, 4, 6, 8, generator=g), torch.randn(2, 4, 6, 8, generator=g)
    return lazy.lift(x.requires_grad_(requires_grad)) * 0.5, lazy.lift(orig) * 0.25


def test_host_operands_that_require_grad_are_still_refused():
    form, known = _forms(True)
    with pytest.raises(lazy.SkrampleHipError, match="a masked step has no backward"):
        lazy.evaluate_masked(form, known, torch.ones(2, 1, 6, 8))
    with torch.no_grad():  # (not recorded: the host executor runs as ever)
        out = lazy.evaluate_masked(form, known, torch.ones(2, 1, 6, 8))
    assert not out.requires_grad


def test_a_mask_that_requires_grad_is_refused():
    form, known = _forms(False)
    with pytest.raises(lazy.SkrampleHipError, match="mask of a masked step has no gradient"):
        lazy.evaluate_masked(form, known, torch.rand(2, 1, 6, 8).requires_grad_())
