"""The row forms of the guided step kernel in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_guided_indexed[_per_sample]` run `guided_kernel_v1<T, K, NOISE, RowForm, false>` (csrc/skr_step_guided.hip) in its
WholeBatch and PerSample forms: the one-trip guided kernel with its scalars -- coefficients, zeta, Philox stream and the guidance scale -- read from a device-resident row
behind the loads.  What the contract promises is visible in the instruction stream: `slot` stays a kernarg scalar compared per unrolled
operand (nothing goes to scratch, no exec masking), operands are 16-byte global loads and both outputs 16-byte global stores.  The
register and occupancy table is printed (run with -s) and recorded in profiles/guided_rows_isa.txt; the brackets asserted at the end
are what that record shows: 8 waves per SIMD up to 4 operands, as the kernarg twin (tests/test_guided_isa.py), never below 3."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

# guided_kernel_v1<T, K, NOISE, RowForm::WholeBatch / PerSample, false>
SYMBOL = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE([12])ELb0EE")
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}
FORMS = {"1": "whole-batch", "2": "per-sample"}  # RowForm::WholeBatch, RowForm::PerSample
VEC = 8  # elements per lane


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "every unrescaled WholeBatch and PerSample instantiation of guided_kernel_v1, selected from the one translation unit, compiled once"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    return {k: v for k, v in found.items() if SYMBOL.search(k)}  # (the census of the whole file: tests/test_guided_isa.py)


def count(lines, *prefixes):
    return sum(1 for l in lines if l.startswith(prefixes))


def test_all_192_instantiations_exist(kernels):
    "3 dtypes x 16 operand counts x noise x the two forms whose row is read behind the loads; no kernarg, no rolling form"
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
        assert count(lines, "global_load_") == count(lines, "global_load_dwordx4"), k  # the row, the index and the seed are scalar loads
        assert count(lines, "global_store_") == count(lines, "global_store_dwordx4"), k


def test_slot_is_a_uniform_comparison_per_operand(kernels):
    "no exec masking; a K-operand kernel holds at least K conditional scalar branches or K * 8 v_cndmask (one per element)"
    for k, (lines, *_) in kernels.items():
        n = int(SYMBOL.search(k).group(2))
        assert not any("saveexec" in l for l in lines), k
        assert count(lines, "s_cbranch_scc", "s_cbranch_vcc") >= n or count(lines, "v_cndmask") >= n * VEC, k


def test_register_and_occupancy_table(kernels):
    """printed for DESIGN.md section 4.7 and profiles/guided_rows_isa.txt (run with -s).  Pinned from that record: up to 4 operands every
    instantiation keeps 8 waves per SIMD (at most 64 VGPRs), the kernarg twin's bracket (tests/test_guided_isa.py); up to 8 operands at
    least 4 -- the noisy forms hold the draw across its branch and sit up to 10 VGPRs above the twin there, one bracket below it at
    K = 8 --, and none falls below 3."""
    names = {v: k for k, v in TYPES.items()}
    print("\nguided_kernel_v1<T, K, NOISE, RowForm, false>: VGPRs (waves per SIMD)")
    rows = {}
    for k, (_, vgprs, *_rest) in kernels.items():
        t, n, nz, f = SYMBOL.search(k).groups()
        rows[(names[t], FORMS[f], int(nz), int(n))] = vgprs
    for t in TYPES:
        for f in FORMS.values():
            for nz in (0, 1):
                print(f"  {t} {f} noise={nz}: " + "  ".join(f"K={n}: {rows[(t, f, nz, n)]} ({waves_per_simd(rows[(t, f, nz, n)])})" for n in range(1, 17)))
    for (t, f, nz, n), vgprs in rows.items():
        waves = waves_per_simd(vgprs)
        assert waves >= 3, (t, f, nz, n, vgprs)
        if n <= 8:
            assert waves >= 4, (t, f, nz, n, vgprs)
        if n <= 4:
            assert waves == 8, (t, f, nz, n, vgprs)
