"""The guided step kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_guided` runs the Kernarg, unrescaled form of `guided_kernel_v1<T, K, NOISE, RowForm, RESCALE>` (csrc/skr_step_guided.hip)
where whole chunks of one dtype allow it.  What
its contract promises is visible in the instruction stream: `slot` is compared per unrolled operand and never indexes the register
arrays (nothing goes to scratch), operands are 16-byte global loads and both outputs 16-byte global stores, and the guidance of an
fp32 tensor stays three instructions per element -- a multiply and an add that a contraction would have fused are both there.  The
register and occupancy table is printed (run with -s) and recorded in profiles/guided_isa.txt; the brackets asserted at the end are
what that record shows.  The file holds every unrescaled form of the guided step and csrc/skr_step_guided_rescaled.hip every rescaled one (the
other five modules select theirs from the same two compiles): this module also pins the census of both files, and that of the statistics
row launches' (csrc/skr_guidance_stats_rows.hip)."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

# guided_kernel_v1<T, K, NOISE, RowForm::Kernarg, false>
SYMBOL = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE0ELb0EE")
ANY_FORM = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE([0-3])ELb([01])EE")  # guided_kernel_v1<T, K, NOISE, RowForm, RESCALE>
GENERAL = re.compile(r"guided_kernel_genI([fd])Lb([01])EE")  # guided_kernel_gen<Acc, RESCALE>
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}
VEC = 8  # elements per lane


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "every Kernarg, unrescaled guided_kernel_v1 instantiation of the one translation unit, compiled once"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    return {k: v for k, v in found.items() if SYMBOL.search(k)}


def count(lines, *prefixes):
    return sum(1 for l in lines if l.startswith(prefixes))


def test_the_two_files_hold_768_one_trip_and_4_general_kernels_and_nothing_else(tmp_path_factory):
    """3 dtypes x 16 operand counts x noise x 4 row forms x rescale, and guided_kernel_gen<float / double, RESCALE>: the unrescaled half
    and the general kernels in skr_step_guided.hip, the rescaled half in skr_step_guided_rescaled.hip"""
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    plain = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    rescaled = kernels_of(compile_asm("skr_step_guided_rescaled.hip", str(tmp_path_factory.mktemp("isa") / "guided_rescaled")))
    half = {(t, str(n), nz, f) for t in TYPES.values() for n in range(1, 17) for nz in "01" for f in "0123"}
    assert {ANY_FORM.search(k).groups() for k in plain if ANY_FORM.search(k)} == {(*key, "0") for key in half}
    assert {ANY_FORM.search(k).groups() for k in rescaled if ANY_FORM.search(k)} == {(*key, "1") for key in half}
    assert {GENERAL.search(k).groups() for k in plain if GENERAL.search(k)} == {(acc, r) for acc in "fd" for r in "01"}
    assert len(plain) == 384 + 4 and len(rescaled) == 384, (len(plain), len(rescaled))
    assert len(set(plain) | set(rescaled)) == 768 + 4


def test_the_statistics_row_file_holds_18_kernels(tmp_path_factory):
    "2 stages x 3 dtypes x the three row forms"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_guidance_stats_rows.hip", str(tmp_path_factory.mktemp("isa") / "stats_rows")))
    stats = re.compile(r"rescale_stats_(spans|final)_rowsI(\w+?)LNS_7RowFormE([123])EE")
    have = {stats.search(k).groups() for k in found if stats.search(k)}
    assert have == {(stage, t, f) for stage in ("spans", "final") for t in TYPES.values() for f in "123"} and len(found) == 18, sorted(found)


def test_all_96_instantiations_exist(kernels):
    "3 dtypes x 16 operand counts x noise; storing p is a uniform branch on the pointer, not a template flag"
    have = {SYMBOL.search(k).groups() for k in kernels}
    want = {(t, str(n), nz) for t in TYPES.values() for n in range(1, 17) for nz in "01"}
    assert have == want and len(kernels) == 96, (sorted(want - have), sorted(have - want))


def test_no_scratch_and_no_private_segment(kernels):
    for k, (lines, _, scratch, private) in kernels.items():
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert not any(l.startswith("scratch_") for l in lines), k


def test_memory_operations_are_global_and_16_bytes_wide(kernels):
    for k, (lines, *_) in kernels.items():
        assert not any(l.startswith("flat_") for l in lines), k
        assert count(lines, "global_load_dwordx4") >= 1 and count(lines, "global_store_dwordx4") >= 1, k
        t, n, _ = SYMBOL.search(k).groups()
        per_vector = 2 if t == "f" else 1  # a lane's 8 elements: one 16-byte access of 16-bit values, two of 32-bit values
        assert count(lines, "global_load_dwordx4") >= per_vector * (int(n) + 1), k  # every operand and cond
        assert count(lines, "global_store_dwordx4") >= 2 * per_vector, k  # out and guided_out


def test_slot_is_a_uniform_comparison_per_operand(kernels):
    "no exec masking; a K-operand kernel holds at least K conditional scalar branches or K * 8 v_cndmask (one per element)"
    for k, (lines, *_) in kernels.items():
        n = int(SYMBOL.search(k).group(2))
        assert not any("saveexec" in l for l in lines), k
        assert count(lines, "s_cbranch_scc", "s_cbranch_vcc") >= n or count(lines, "v_cndmask") >= n * VEC, k


def test_fp32_guidance_is_not_contracted(kernels):
    "at least 8 v_mul_f32 and 8 v_add_f32 / v_sub_f32 in every fp32 instantiation: g * d and u + m stay two instructions per element"
    seen = 0
    for k, (lines, *_) in kernels.items():
        if SYMBOL.search(k).group(1) != TYPES["fp32"]:
            continue
        seen += 1
        assert count(lines, "v_mul_f32") >= VEC, (k, count(lines, "v_mul_f32"))
        assert count(lines, "v_add_f32", "v_sub_f32") >= VEC, (k, count(lines, "v_add_f32", "v_sub_f32"))
    assert seen == 32


def test_register_and_occupancy_table(kernels):
    """printed for DESIGN.md section 4.7 and profiles/guided_isa.txt (run with -s).  Pinned from that record: up to 4 operands every
    instantiation keeps 8 waves per SIMD (at most 64 VGPRs), up to 8 operands at least 5, and none falls below 3."""
    names = {v: k for k, v in TYPES.items()}
    print("\nguided_kernel_v1<T, K, NOISE, Kernarg, false>: VGPRs (waves per SIMD)")
    rows = {}
    for k, (_, vgprs, *_rest) in kernels.items():
        t, n, nz = SYMBOL.search(k).groups()
        rows[(names[t], int(nz), int(n))] = vgprs
    for t in TYPES:
        for nz in (0, 1):
            print(f"  {t} noise={nz}: " + "  ".join(f"K={n}: {rows[(t, nz, n)]} ({waves_per_simd(rows[(t, nz, n)])})" for n in range(1, 17)))
    for (t, nz, n), vgprs in rows.items():
        waves = waves_per_simd(vgprs)
        assert waves >= 3, (t, nz, n, vgprs)
        if n <= 8:
            assert waves >= 5, (t, nz, n, vgprs)
        if n <= 4:
            assert waves == 8, (t, nz, n, vgprs)
