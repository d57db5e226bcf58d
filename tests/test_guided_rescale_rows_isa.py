"""The rescaled guided row kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_guided_rescaled_indexed[_per_sample]` run `guided_kernel_v1<T, K, NOISE, RowForm, true>` (csrc/skr_step_guided_kernel.h, compiled in csrc/skr_step_guided_rescaled.hip) in its
WholeBatch and PerSample forms: their unrescaled twins with one more decision taken from the row -- whether it rescales.  What
the contract promises is visible in the instruction stream, as that of its twin is (tests/test_guided_rows_isa.py): `slot` stays a kernarg
scalar compared per unrolled operand and the `phi` test is a scalar branch (nothing goes to scratch, exec is never masked); operands and
cond are 16-byte global loads, both outputs 16-byte global stores; beside them there is at most the factor, one 16-bit element from a
uniform address.  The VGPR and occupancy table is printed beside `guided_kernel_v1<T, K, NOISE, RowForm, false>` -- run with -s -- and
recorded in profiles/guided_rescale_rows_isa.txt; the brackets asserted at the end are what that record shows.

`skr_guidance_rescale_factor_indexed[_per_sample]` run two kernels (the WholeBatch and PerSample forms of csrc/skr_guidance_stats_rows.hip).  Both end the workgroups of an
unrescaled row before their first vector-memory instruction, neither spills, and every vector load of either is 16 bytes wide (the index,
the row and the pivots are scalar loads)."""

import os
import re

import pytest
from isa_cases import HIPCC, ROOT, compile_asm, kernels_of, waves_per_simd

VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")
BRANCH = ("s_cbranch_scc", "s_cbranch_vcc")
SYMBOL = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE([12])ELb1EE")  # guided_kernel_v1<T, K, NOISE, WholeBatch / PerSample, true>
TWIN = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE([12])ELb0EE")  # guided_kernel_v1<T, K, NOISE, WholeBatch / PerSample, false>
STATS = re.compile(r"rescale_stats_(spans|final)_rowsI(\w+?)LNS_7RowFormE([12])EE")  # rescale_stats_{spans,final}_rows<T, WholeBatch / PerSample>
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}
FORMS = {"1": "whole-batch", "2": "per-sample"}  # RowForm::WholeBatch, RowForm::PerSample
RECORD = os.path.join(ROOT, "profiles", "guided_rescale_rows_isa.txt")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "every rescaled WholeBatch and PerSample instantiation of guided_kernel_v1, selected from their translation unit, compiled once"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided_rescaled.hip", str(tmp_path_factory.mktemp("isa") / "guided_rescaled")))
    return {k: v for k, v in found.items() if SYMBOL.search(k)}  # (the census of the whole file: tests/test_guided_isa.py)


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    return {TWIN.search(k).groups(): v for k, v in found.items() if TWIN.search(k)}


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    "both stages of the statistics row launch, every dtype, both forms"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_guidance_stats_rows.hip", str(tmp_path_factory.mktemp("isa") / "stats_rows")))
    return {k: v for k, v in found.items() if STATS.search(k)}  # (the census of the whole file: tests/test_guided_isa.py)


def count(lines, *prefixes):
    return sum(1 for l in lines if l.startswith(prefixes))


def exits_before_vector_memory(lines) -> bool:
    "a conditional scalar branch, ahead of the first vector-memory instruction, whose target runs into s_endpgm without touching vector memory"
    first = next(i for i, l in enumerate(lines) if VMEM.match(l))
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.startswith(".LBB") and l.endswith(":")}
    for l in lines[:first]:
        if l.startswith(BRANCH):
            tail = [t for t in lines[labels[l.split()[-1]] :] if not t.startswith(".LBB")]
            if tail[0] == "s_endpgm":
                return True
    return False


def test_all_192_instantiations_exist(kernels):
    "3 dtypes x 16 operand counts x noise x the two forms whose row is read behind the loads, and nothing else"
    have = {SYMBOL.search(k).groups() for k in kernels}
    want = {(t, str(n), nz, f) for t in TYPES.values() for n in range(1, 17) for nz in "01" for f in FORMS}
    assert have == want and len(kernels) == 192, (sorted(want - have), sorted(have - want))


def test_no_scratch_and_no_private_segment(kernels):
    for k, (lines, _, scratch, private) in kernels.items():
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert not any(l.startswith("scratch_") for l in lines), k


def test_memory_operations_are_global_and_16_bytes_wide(kernels):
    for k, (lines, *_) in kernels.items():
        assert not any(l.startswith("flat_") for l in lines), k
        t, n, *_ = SYMBOL.search(k).groups()
        per_vector = 2 if t == "f" else 1  # a lane's 8 elements: one 16-byte access of 16-bit values, two of 32-bit values
        assert count(lines, "global_load_dwordx4") >= per_vector * (int(n) + 1), k  # every operand and cond
        assert count(lines, "global_store_dwordx4") >= 2 * per_vector, k  # out and guided_out
        assert count(lines, "global_store_") == count(lines, "global_store_dwordx4"), k
        # beside the 16-byte loads: at most the factor, one element of T from a uniform address (a 16-bit value has no scalar load)
        assert count(lines, "global_load_") - count(lines, "global_load_dwordx4") <= (0 if t == "f" else 1), k


def test_the_loads_lead_and_the_factor_sits_behind_the_phi_branch(kernels):
    "every 16-byte load of operands and cond precedes the first conditional branch; a 16-bit factor's load follows one"
    for k, (lines, *_) in kernels.items():
        t, n, *_ = SYMBOL.search(k).groups()
        per_vector = 2 if t == "f" else 1
        branch = next(i for i, l in enumerate(lines) if l.startswith(BRANCH))
        assert count(lines[:branch], "global_load_dwordx4") == per_vector * (int(n) + 1), k
        assert count(lines[:branch], "global_load_") == count(lines[:branch], "global_load_dwordx4"), k


def test_the_phi_test_and_the_slot_test_are_scalar_branches(kernels):
    "no exec masking anywhere; a K-operand kernel has at least K + 1 conditional scalar branches (the phi test and one per operand)"
    for k, (lines, *_) in kernels.items():
        assert not any("saveexec" in l for l in lines), k
        assert count(lines, *BRANCH) >= int(SYMBOL.search(k).group(2)) + 1, k


def recorded_short() -> list:
    "the instantiations the record lists as a waves-per-SIMD bracket below their twin"
    with open(RECORD) as fh:
        line = next(l for l in fh if l.strip().startswith("fewer waves per SIMD than the twin:"))
    listed = line.split(":", 1)[1].strip()
    return [] if listed == "none" else [w.strip() for w in listed.split(",")]


def test_register_and_occupancy_table_against_the_unrescaled_twins(kernels, twins):
    """printed for DESIGN.md section 4.7 and profiles/guided_rescale_rows_isa.txt (run with -s).  At least 3 waves per SIMD everywhere, at
    least 4 up to 8 operands, 8 up to 4 operands -- the twin's own brackets (tests/test_guided_rows_isa.py) -- except 7 for the listed
    fp32 noise forms at K = 4; the instantiations that sit a bracket below their unrescaled twin are the ones the record lists
    by name."""
    names = {v: k for k, v in TYPES.items()}
    print("\nVGPRs (waves per SIMD): guided_kernel_v1<T, K, NOISE, RowForm, true> vs guided_kernel_v1<T, K, NOISE, RowForm, false>")
    short = []
    for key in sorted((SYMBOL.search(k).groups() for k in kernels), key=lambda g: (g[0], g[3], g[2], int(g[1]))):
        symbol = next(k for k in kernels if SYMBOL.search(k).groups() == key)
        assert key in twins, key
        mine, theirs = kernels[symbol][1], twins[key][1]
        n = int(key[1])
        what = f"{names[key[0]]} {FORMS[key[3]]} K={n:2d} noise={key[2]}"
        print(f"  {what}: {mine:3d} ({waves_per_simd(mine)}) vs {theirs:3d} ({waves_per_simd(theirs)})")
        if waves_per_simd(mine) < waves_per_simd(theirs):
            short.append(what)
        waves = waves_per_simd(mine)
        assert waves >= 3, (what, mine)
        if n <= 8:
            assert waves >= 4, (what, mine)
        if n <= 4:  # 8, except where the record lists the instantiation a bracket below its twin (the fp32 noise forms at K = 4: 66 VGPRs)
            assert waves == 8 or (waves == 7 and what in short), (what, mine)
    print("  fewer waves per SIMD than the twin:", ", ".join(short) if short else "none")
    assert short == recorded_short(), (short, recorded_short())


def test_statistics_kernels_exit_early_spill_nothing_and_load_16_bytes(stats):
    have = {STATS.search(k).groups() for k in stats}
    assert have == {(stage, t, f) for stage in ("spans", "final") for t in TYPES.values() for f in FORMS} and len(stats) == 12, sorted(have)
    for k, (lines, _, scratch, private) in stats.items():
        assert exits_before_vector_memory(lines), k
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert not any(l.startswith(("scratch_", "flat_")) for l in lines), k
        assert count(lines, "global_load_") == count(lines, "global_load_dwordx4") >= 1, k  # the index, the row and the pivots are scalar loads
