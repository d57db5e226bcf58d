"""The masked channels-last one-trip kernel in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`masked_kernel_cl1<T, K, C, NOISE>` (csrc/skr_step_masked_channels_last.hip) is step_kernel_cl1 with masked_kernel_v1's two
coefficient sets and a per-pixel mask load.  This module compiles the file with the library's own flags and checks, for every
instantiation, that nothing spills, that no memory operation is a flat one, that the operands move as 16-byte vectors, and that the
draw is step_kernel_cl1's: the same DPP / swizzle counts per channel count (none without a draw), no LDS memory, and, against the
contiguous twin `masked_kernel_v1<T, 4, true, Kernarg>` of csrc/skr_step_masked.hip, not a single extra full-width multiply of the
Philox rounds.  The register table it prints is the one in DESIGN.md section 4.6; nothing about occupancy is asserted beyond "no
scratch"."""

import re

import pytest
from isa_cases import CXXFILT, HIPCC, WIDE_MUL, named, waves_per_simd, wide_multiplies
from test_channels_last_isa import EXCHANGE  # (DPP quad permutes, ds_swizzle) of step_kernel_cl1

ONE_TRIP = re.compile(r"masked_kernel_cl1<skr::(bf16_t|f16_t), (\d+), (\d+), (true|false)>")
TWIN = "masked_kernel_v1<skr::{t}, 4, true, (skr::RowForm)0>"
QUIET_TWIN = "masked_kernel_v1<skr::{t}, 4, false, (skr::RowForm)0>"


@pytest.fixture(scope="module")
def mine(tmp_path_factory):
    if HIPCC is None or CXXFILT is None:
        pytest.skip("no hipcc / c++filt on this box")
    return named("skr_step_masked_channels_last.hip", str(tmp_path_factory.mktemp("isa") / "mcl"))


@pytest.fixture(scope="module")
def masked(tmp_path_factory):
    if HIPCC is None or CXXFILT is None:
        pytest.skip("no hipcc / c++filt on this box")
    return named("skr_step_masked.hip", str(tmp_path_factory.mktemp("isa") / "masked"))


def one_trip(kernels):
    found = {}
    for name, body in kernels.items():
        m = ONE_TRIP.search(name)
        if m:
            found[(m.group(1), int(m.group(2)), int(m.group(3)), m.group(4) == "true")] = body
    return found


def test_all_96_instantiations_exist(mine):
    want = {(t, k, c, nz) for t in ("bf16_t", "f16_t") for k in range(1, 9) for c in (4, 8, 16) for nz in (False, True)}
    assert len(want) == 96 and set(one_trip(mine)) == want


def test_no_scratch_no_flat_memory_operation_and_16_byte_vectors(mine):
    for key, (lines, vgprs, scratch, private) in one_trip(mine).items():
        assert scratch == 0 and private == 0, (key, scratch, private)
        assert not any(l.startswith("flat_") for l in lines), key
        assert any(l.startswith("global_load_dwordx4") for l in lines) and any(l.startswith("global_store_dwordx4") for l in lines), key
        assert sum(1 for l in lines if l.startswith("global_load_dwordx4")) >= key[1], key  # a vector load per operand


def test_the_mask_is_one_narrow_load_per_lane(mine):
    "two 16-bit elements in one dword at C = 4, one 16-bit element otherwise"
    for (t, k, c, nz), (lines, _, _, _) in one_trip(mine).items():
        dword = sum(1 for l in lines if l.startswith("global_load_dword ") or l.startswith("global_load_dword\t"))
        short = sum(1 for l in lines if l.startswith(("global_load_ushort", "global_load_short", "global_load_sshort")))
        assert (dword, short) == ((1, 0) if c == 4 else (0, 1)), (t, k, c, nz, dword, short)


def test_the_exchange_is_step_kernel_cl1s_and_runs_in_registers(mine):
    "DPP quad permutes for lane bits 0 and 1, ds_swizzle for bit 2; no LDS memory, no bpermute; a launch without a draw has none of it"
    for (t, k, c, nz), (lines, _, _, _) in one_trip(mine).items():
        dpp = sum(1 for l in lines if "quad_perm" in l)
        swizzle = sum(1 for l in lines if l.startswith("ds_swizzle_b32"))
        assert not any(l.startswith(("ds_read", "ds_write", "ds_bpermute", "ds_permute")) for l in lines), (t, k, c, nz)
        assert (dpp, swizzle) == (EXCHANGE[c] if nz else (0, 0)), (t, k, c, nz, dpp, swizzle)


def test_the_draw_costs_no_philox_multiply_and_the_register_table(mine, masked):
    "two whole blocks per lane, as in the contiguous masked kernel: no more 32 x 32 multiplies than its twin has"
    kernels = one_trip(mine)
    rows = []
    for t in ("bf16_t", "f16_t"):
        twin_lines, twin_vgprs, _, _ = next(body for name, body in masked.items() if TWIN.format(t=t) in name)
        quiet_lines = next(body for name, body in masked.items() if QUIET_TWIN.format(t=t) in name)[0]
        which = tuple(w for w in WIDE_MUL if wide_multiplies(twin_lines, (w,)))  # whichever the twin compiles to
        assert which, t
        twin_muls = wide_multiplies(twin_lines, which)
        assert 30 <= twin_muls <= 40, twin_muls  # 2 blocks x 10 rounds x 2 products, less what constant folding takes
        for c in (4, 8, 16):
            for nz in (True, False):
                lines, vgprs, _, _ = kernels[(t, 4, c, nz)]
                muls = wide_multiplies(lines, WIDE_MUL)  # (every wide multiply of the kernel, in either spelling)
                rows.append(f"{t:7s} C={c:<2d} {'draw   ' if nz else 'no draw'} NumVgprs {vgprs:3d} (twin {twin_vgprs:3d})  waves/SIMD {waves_per_simd(vgprs)} (twin {waves_per_simd(twin_vgprs)})"
                            f"  wide multiplies {muls:2d} (twin {twin_muls:2d})  instructions {len(lines):3d} (twin {len(twin_lines):3d})")  # fmt: skip
                if nz:
                    assert muls <= twin_muls, rows[-1]
                else:  # what is left without a draw is the mask index's remainder, which the twin without a draw has too
                    assert muls <= wide_multiplies(quiet_lines, WIDE_MUL), rows[-1]
    print("\n" + "\n".join(rows))
