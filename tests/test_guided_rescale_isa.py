"""The rescaled guided step kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_guided_rescaled` runs `guided_kernel_v1<T, K, NOISE, RowForm::Kernarg, true>` (csrc/skr_step_guided_kernel.h, compiled in csrc/skr_step_guided_rescaled.hip) where whole chunks
of one dtype and samples of whole chunks allow it.  It keeps the shape of its unrescaled twin (RESCALE false), and that is visible in the instruction stream:
nothing goes to scratch, operands and cond are 16-byte global loads and both outputs 16-byte global stores, `slot` is a uniform
comparison (no exec masking), and for an fp32 tensor the seven operations of  phi * (p * r) + psi * p  over  p = u + g * (c - u)  stay
seven instructions per element -- four multiplies and three additions that a contraction would have fused are all there.  The register
and occupancy table is printed beside that of the unrescaled twins (run with -s) and recorded in profiles/guided_rescale_isa.txt;
the brackets asserted at the end are what that record shows.  Registers, memory-operation widths and arithmetic counts only."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

# guided_kernel_v1<T, K, NOISE, RowForm::Kernarg, true> and its twin guided_kernel_v1<T, K, NOISE, RowForm::Kernarg, false>
SYMBOL = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE0ELb1EE")
TWIN = re.compile(r"guided_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE0ELb0EE")
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}
VEC = 8  # elements per lane


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "every Kernarg, rescaled guided_kernel_v1 instantiation of their translation unit, compiled once"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_step_guided_rescaled.hip", str(tmp_path_factory.mktemp("isa") / "guided_rescaled")))
    return {k: v for k, v in found.items() if SYMBOL.search(k)}


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    found = kernels_of(compile_asm("skr_step_guided.hip", str(tmp_path_factory.mktemp("isa") / "guided")))
    return {TWIN.search(k).groups(): v for k, v in found.items() if TWIN.search(k)}


def count(lines, *prefixes):
    return sum(1 for l in lines if l.startswith(prefixes))


def test_all_96_instantiations_exist(kernels):
    "3 dtypes x 16 operand counts x noise; storing p' is a uniform branch on the pointer, not a template flag"
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
        t, n, _ = SYMBOL.search(k).groups()
        per_vector = 2 if t == "f" else 1  # a lane's 8 elements: one 16-byte access of 16-bit values, two of 32-bit values
        assert count(lines, "global_load_dwordx4") >= per_vector * (int(n) + 1), k  # every operand and cond
        assert count(lines, "global_store_dwordx4") >= 2 * per_vector, k  # out and guided_out


def test_no_exec_masking(kernels):
    for k, (lines, *_) in kernels.items():
        assert not any("saveexec" in l for l in lines), k


def test_fp32_rescale_is_not_contracted(kernels):
    "g * d, p * r, phi * resc, psi * p: 4 x 8 v_mul_f32; c - u, u + m, a + b: 3 x 8 v_add_f32 / v_sub_f32, in every fp32 instantiation"
    seen = 0
    for k, (lines, *_) in kernels.items():
        if SYMBOL.search(k).group(1) != TYPES["fp32"]:
            continue
        seen += 1
        assert count(lines, "v_mul_f32") >= 4 * VEC, (k, count(lines, "v_mul_f32"))
        assert count(lines, "v_add_f32", "v_sub_f32") >= 3 * VEC, (k, count(lines, "v_add_f32", "v_sub_f32"))
    assert seen == 32


def test_register_and_occupancy_table(kernels, twins):
    """printed for DESIGN.md section 4.7 and profiles/guided_rescale_isa.txt (run with -s), each instantiation beside its guided_kernel_v1
    twin.  Pinned from that record: one instantiation sits a waves-per-SIMD bracket below its twin -- bf16 with noise at 14 operands, 130
    against 128 VGPRs -- and no other, and the twin's brackets hold: 8 waves per SIMD up to 4 operands, at least 5 up to 8, never below 3."""
    names = {v: k for k, v in TYPES.items()}
    print("\nguided_kernel_v1<T, K, NOISE, Kernarg, true>: VGPRs (waves per SIMD) | guided_kernel_v1<T, K, NOISE, Kernarg, false> twin")
    rows = {}
    for k, (_, vgprs, *_rest) in kernels.items():
        t, n, nz = SYMBOL.search(k).groups()
        rows[(names[t], int(nz), int(n))] = (vgprs, twins[(t, n, nz)][1])
    for t in TYPES:
        for nz in (0, 1):
            print(f"  {t} noise={nz}: " + "  ".join(f"K={n}: {rows[(t, nz, n)][0]} ({waves_per_simd(rows[(t, nz, n)][0])}) | {rows[(t, nz, n)][1]} ({waves_per_simd(rows[(t, nz, n)][1])})" for n in range(1, 17)))
    below = {key: (own, twin) for key, (own, twin) in rows.items() if waves_per_simd(own) < waves_per_simd(twin)}
    assert set(below) <= {("bf16", 1, 14)}, below  # the one the record shows: 130 against 128 VGPRs, 3 waves against 4
    for (t, nz, n), (vgprs, _) in rows.items():
        waves = waves_per_simd(vgprs)
        assert waves >= 3, (t, nz, n, vgprs)
        if n <= 8:
            assert waves >= 5, (t, nz, n, vgprs)
        if n <= 4:
            assert waves == 8, (t, nz, n, vgprs)
