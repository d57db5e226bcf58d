"""The per-sample step kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_indexed_per_sample` runs the `RowForm::PerSample` instantiations of the one-trip kernels (csrc/skr_step_fast.hip:
step_kernel_k1 / _k2 / _rk1): the whole-batch (`RowForm::WholeBatch`) table instantiations with the row chosen by the workgroup's
sample.  A workgroup belongs to one sample, so the per-sample index and the row it names must be fetched by scalar loads, exactly as the whole-batch form fetches
`index[0]` and its row -- as per-lane vector loads they would add vector-memory traffic to an HBM-bound kernel.  This module compiles
the file with the library's own flags and compares every per-sample instantiation with its whole-batch twin: no more vector-memory
loads, no scratch, the same occupancy."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

VLOAD = re.compile(r"^(global|flat|buffer|scratch)_load")
SLOAD = re.compile(r"^s_(buffer_)?load")
# the mangled RowForm argument of the three kernels (skr_step_common.h): Kernarg 0, WholeBatch 1, PerSample 2, Rolling 3
PER_SAMPLE, WHOLE_BATCH = "LNS_7RowFormE2E", "LNS_7RowFormE1E"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "{symbol: (instructions and labels, VGPRs, scratch bytes, private segment size)} of every kernel of skr_step_fast.hip"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    return kernels_of(compile_asm("skr_step_fast.hip", str(tmp_path_factory.mktemp("isa") / "fast")))


def pairs(kernels):
    found = [(k, k.replace(PER_SAMPLE, WHOLE_BATCH)) for k in kernels if PER_SAMPLE in k]
    for k, twin in found:
        assert twin in kernels, ("no whole-batch twin", k)
    return found


def test_every_table_instantiation_has_a_per_sample_form(kernels):
    "the whole-batch instantiations of the three kernels (RowForm: last-but-BLK / last-but-NT / last argument), and their per-sample forms, one to one"
    found = pairs(kernels)
    for name in ("step_kernel_k1I", "step_kernel_k2I", "step_kernel_rk1I"):
        assert sum(1 for k, _ in found if name in k) >= 20, name
    tabs = set()
    for k in kernels:
        if re.search(r"14step_kernel_k1I.*LNS_7RowFormE1EEEvNS_11OneTripArgs", k) or re.search(r"15step_kernel_rk1I.*LNS_7RowFormE1ELi\d+EEEvNS_13RkOneTripArgs", k) or re.search(r"14step_kernel_k2I.*LNS_7RowFormE1ELb0EEEvNS_10TwoOutArgs", k):
            tabs.add(k)
    assert tabs == {twin for _, twin in found}, sorted(tabs ^ {twin for _, twin in found})[:4]


def test_row_and_index_fetches_stay_scalar(kernels):
    "(a) no per-sample instantiation has more vector-memory loads than its twin; the index and row fetches show up as scalar loads"
    for k, twin in pairs(kernels):
        mine, theirs = kernels[k][0], kernels[twin][0]
        count = lambda lines, what: sum(1 for l in lines if what.match(l))  # noqa: E731
        assert count(mine, VLOAD) <= count(theirs, VLOAD), (k, count(mine, VLOAD), count(theirs, VLOAD))
        assert count(mine, SLOAD) >= 3, k  # kernarg, index entry, row
        assert any(l.startswith("v_readfirstlane") for l in mine), k  # the sample id of the dividing chunk -> sample map


def test_no_scratch_and_the_twins_occupancy(kernels):
    "(b) private segment size 0, and the VGPR count in the occupancy bracket of the twin"
    for k, twin in pairs(kernels):
        _, vgprs, scratch, private = kernels[k]
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert waves_per_simd(vgprs) >= waves_per_simd(kernels[twin][1]), (k, vgprs, kernels[twin][1])
