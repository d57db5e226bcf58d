"""The guided rolling step kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_guided_rolling` runs `guided_kernel_v1<T, K, NOISE, RowForm::Rolling, false>` (csrc/skr_step_guided.hip): the per-sample
row form of the guided kernel with the statement order of the rolling forms.  Its contract is visible in the instruction stream, as that of the
other rolling kernels is (tests/test_rolling_isa.py, tests/test_masked_rolling_isa.py): a workgroup of an inactive sample ends before its
first vector-memory instruction, every decision taken from the sample's row and the `slot` test of each unrolled operand is a scalar
branch with exec never masked, operands and cond are 16-byte global loads, both outputs 16-byte global stores, and nothing spills.  The
VGPR and occupancy table is printed beside the per-sample twins `guided_kernel_v1<T, K, NOISE, RowForm::PerSample, false>` of the same
file -- run with -s -- and recorded in profiles/guided_rolling_isa.txt; the brackets asserted at the end are
what that record shows."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")
BRANCH = ("s_cbranch_scc", "s_cbranch_vcc")
SYMBOL = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE3ELb0EE")  # guided_kernel_v1<T, K, NOISE, RowForm::Rolling, false>
TWIN = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE2ELb0EE")  # guided_kernel_v1<T, K, NOISE, RowForm::PerSample, false>
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "every unrescaled Rolling instantiation of guided_kernel_v1, selected from the one translation unit, compiled once"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    return {k: v for k, v in found.items() if SYMBOL.search(k)}  # (the census of the whole file: tests/test_guided_isa.py)


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    return {TWIN.search(k).groups(): v for k, v in found.items() if TWIN.search(k)}


def count(lines, *prefixes):
    return sum(1 for l in lines if l.startswith(prefixes))


def test_all_96_instantiations_exist(kernels):
    "3 dtypes x 16 operand counts x noise, and nothing else"
    have = {SYMBOL.search(k).groups() for k in kernels}
    want = {(t, str(n), nz) for t in TYPES.values() for n in range(1, 17) for nz in "01"}
    assert have == want and len(kernels) == 96, (sorted(want - have), sorted(have - want))


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


def test_no_scratch_and_no_private_segment(kernels):
    for k, (lines, _, scratch, private) in kernels.items():
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert not any(l.startswith("scratch_") for l in lines), k


def test_memory_operations_are_global_and_16_bytes_wide(kernels):
    for k, (lines, *_) in kernels.items():
        assert not any(l.startswith("flat_") for l in lines), k
        t, n, _ = SYMBOL.search(k).groups()
        per_vector = 2 if t == "f" else 1  # a lane's 8 elements: one 16-byte access of 16-bit values, two of 32-bit values
        assert count(lines, "global_load_dwordx4") >= per_vector * (int(n) + 1), k  # every operand and cond
        assert count(lines, "global_store_dwordx4") >= 2 * per_vector, k  # out and guided_out
        assert count(lines, "global_load_") == count(lines, "global_load_dwordx4"), k  # the row, the index and the seed are scalar loads
        assert count(lines, "global_store_") == count(lines, "global_store_dwordx4"), k


def test_row_decisions_and_the_slot_test_are_scalar_branches(kernels):
    "no exec masking anywhere; a K-operand kernel has at least K + 1 conditional scalar branches (the exit and one per operand)"
    for k, (lines, *_) in kernels.items():
        assert not any("saveexec" in l for l in lines), k
        assert count(lines, *BRANCH) >= int(SYMBOL.search(k).group(2)) + 1, k


def test_register_and_occupancy_table_against_the_per_sample_twins(kernels, twins):
    """printed for DESIGN.md section 4.7 and profiles/guided_rolling_isa.txt (run with -s).  Pinned from that record: the brackets of the
    per-sample twins' own record (tests/test_guided_rows_isa.py) hold here too -- 8 waves per SIMD up to 4 operands, at least 4 up to 8,
    never below 3 -- and no instantiation has fewer waves per SIMD than its twin."""
    names = {v: k for k, v in TYPES.items()}
    print("\nVGPRs (waves per SIMD): guided_kernel_v1<T, K, NOISE, Rolling, false> vs guided_kernel_v1<T, K, NOISE, PerSample, false>")
    short = []
    for key in sorted((SYMBOL.search(k).groups() for k in kernels), key=lambda g: (g[0], g[2], int(g[1]))):
        symbol = next(k for k in kernels if SYMBOL.search(k).groups() == key)
        assert key in twins, key
        mine, theirs = kernels[symbol][1], twins[key][1]
        n = int(key[1])
        what = f"{names[key[0]]} K={n:2d} noise={key[2]}"
        print(f"  {what}: {mine:3d} ({waves_per_simd(mine)}) vs {theirs:3d} ({waves_per_simd(theirs)})")
        if waves_per_simd(mine) < waves_per_simd(theirs):
            short.append(what)
        waves = waves_per_simd(mine)
        assert waves >= 3, (what, mine)
        if n <= 8:
            assert waves >= 4, (what, mine)
        if n <= 4:
            assert waves == 8, (what, mine)
    print("  fewer waves per SIMD than the twin:", ", ".join(short) if short else "none")
    assert not short, short
