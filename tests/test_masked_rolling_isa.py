"""The masked rolling step kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_masked_rolling` runs `masked_kernel_v1<T, K, NOISE, RowForm::Rolling>` (csrc/skr_step_masked.hip).  Its contract is
visible in the instruction stream, as that of the `RowForm::Rolling` step kernels is (tests/test_rolling_isa.py): a workgroup of an inactive
sample ends before its first vector-memory instruction, every decision taken from the sample's row is a scalar branch with exec never
masked, operands are global loads, and nothing spills.  The VGPR counts are printed beside those of the per-sample twins
`masked_kernel_v1<T, K, NOISE, RowForm::PerSample>`, the same template compiled once, for DESIGN.md section 4.6; no occupancy bracket
is asserted.  The census counts every one-trip instantiation of the template: 3 dtypes x 16 operand counts x noise x 4 row forms."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")
BRANCH = ("s_cbranch_scc", "s_cbranch_vcc")
# masked_kernel_v1<T, K, NOISE, RowForm F>; RowForm (skr_step_common.h): Kernarg 0, WholeBatch 1, PerSample 2, Rolling 3
ONE_TRIP = re.compile(r"masked_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE([0-3])EE")
SYMBOL = re.compile(r"masked_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE3EE")
TWIN = re.compile(r"masked_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE2EE")
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}


@pytest.fixture(scope="module")
def one_trip(tmp_path_factory):
    "every masked_kernel_v1 instantiation of the one translation unit, compiled once"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_masked.hip", str(tmp_path_factory.mktemp("isa") / "masked")))
    return {k: v for k, v in found.items() if ONE_TRIP.search(k)}


@pytest.fixture(scope="module")
def kernels(one_trip):
    return {k: v for k, v in one_trip.items() if SYMBOL.search(k)}


@pytest.fixture(scope="module")
def twins(one_trip):
    return {TWIN.search(k).groups(): v for k, v in one_trip.items() if TWIN.search(k)}


def test_all_96_instantiations_exist(kernels, one_trip):
    have = {SYMBOL.search(k).groups() for k in kernels}
    want = {(t, str(n), nz) for t in TYPES.values() for n in range(1, 17) for nz in "01"}
    assert have == want and len(kernels) == 96, (sorted(want - have), sorted(have - want))
    have = {ONE_TRIP.search(k).groups() for k in one_trip}
    want = {(t, str(n), nz, f) for t in TYPES.values() for n in range(1, 17) for nz in "01" for f in "0123"}
    assert have == want and len(one_trip) == 384, (sorted(want - have), sorted(have - want))


def test_inactive_exit_precedes_the_first_vector_memory_instruction(kernels):
    "a conditional scalar branch whose target runs into s_endpgm without touching vector memory, ahead of the first vector-memory instruction"
    for k, (lines, *_) in kernels.items():
        first = next(i for i, l in enumerate(lines) if VMEM.match(l))
        labels = {l[:-1]: i for i, l in enumerate(lines) if l.startswith(".LBB") and l.endswith(":")}
        exits = False
        for l in lines[:first]:
            if l.startswith(BRANCH):
                tail = [t for t in lines[labels[l.split()[-1]] :] if not t.startswith(".LBB")]
                exits = exits or tail[0] == "s_endpgm"
        assert exits, (k, lines[:first][-12:])


def test_row_decisions_are_scalar_branches(kernels):
    "no exec masking anywhere; a K-operand kernel has at least K + 1 conditional scalar branches (the exit and one per operand)"
    for k, (lines, *_) in kernels.items():
        assert not any("saveexec" in l for l in lines), k
        assert sum(1 for l in lines if l.startswith(BRANCH)) >= int(SYMBOL.search(k).group(2)) + 1, k


def test_operands_are_global_loads(kernels):
    for k, (lines, *_) in kernels.items():
        assert not any(l.startswith("flat_") for l in lines), k
        assert sum(1 for l in lines if l.startswith("global_load")) >= int(SYMBOL.search(k).group(2)) + 1, k  # every operand and the mask


def test_no_scratch(kernels):
    for k, (lines, _, scratch, private) in kernels.items():
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert not any(l.startswith("scratch_") for l in lines), k


def test_vgpr_table_against_the_per_sample_twins(kernels, twins):
    "printed for DESIGN.md section 4.6 (run with -s); every kernel has a twin, and nothing else is asserted: no occupancy bracket"
    names = {v: k for k, v in TYPES.items()}
    print("\nVGPRs (waves per SIMD): masked_kernel_v1<..., Rolling> vs masked_kernel_v1<..., PerSample>")
    short = []
    for key in sorted((SYMBOL.search(k).groups() for k in kernels), key=lambda g: (g[0], g[2], int(g[1]))):
        symbol = next(k for k in kernels if SYMBOL.search(k).groups() == key)
        assert key in twins, key
        mine, theirs = kernels[symbol][1], twins[key][1]
        what = f"{names[key[0]]} K={int(key[1]):2d} noise={key[2]}"
        print(f"  {what}: {mine:3d} ({waves_per_simd(mine)}) vs {theirs:3d} ({waves_per_simd(theirs)})")
        if waves_per_simd(mine) < waves_per_simd(theirs):
            short.append(what)
    print("  fewer waves per SIMD than the twin:", ", ".join(short) if short else "none")
