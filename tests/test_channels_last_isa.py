"""The channels-last one-trip step kernel in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`step_kernel_cl1<T, K, C>` (csrc/skr_step_channels_last.hip) is step_kernel_k1's unpaced Kernarg form with the Philox draw spread over
lane groups: every lane draws two WHOLE blocks, as the contiguous kernel does, and the group exchanges normals in registers.  This
module compiles the file with the library's own flags and checks, for every instantiation, that nothing spills and no memory operation
is a flat one, and, against the contiguous twin `step_kernel_k1<T, 4, true, false, false, Kernarg>` of csrc/skr_step_fast.hip, that the
exchange did not cost a single extra full-width multiply of the Philox rounds."""

import re

import pytest
from isa_cases import CXXFILT, HIPCC, WIDE_MUL, named, waves_per_simd, wide_multiplies

ONE_TRIP = re.compile(r"step_kernel_cl1<skr::(bf16_t|f16_t), (\d+), (\d+)>")
TWIN = "step_kernel_k1<skr::{t}, 4, true, false, false, (skr::RowForm)0>"
EXCHANGE = {4: (4, 0), 8: (8, 0), 16: (4, 4)}  # (DPP quad permutes, ds_swizzle) of cl_draw8 per channel count


@pytest.fixture(scope="module")
def mine(tmp_path_factory):
    if HIPCC is None or CXXFILT is None:
        pytest.skip("no hipcc / c++filt on this box")
    return named("skr_step_channels_last.hip", str(tmp_path_factory.mktemp("isa") / "cl"))


@pytest.fixture(scope="module")
def fast(tmp_path_factory):
    if HIPCC is None or CXXFILT is None:
        pytest.skip("no hipcc / c++filt on this box")
    return named("skr_step_fast.hip", str(tmp_path_factory.mktemp("isa") / "fast"))


def one_trip(kernels):
    found = {}
    for name, body in kernels.items():
        m = ONE_TRIP.search(name)
        if m:
            found[(m.group(1), int(m.group(2)), int(m.group(3)))] = body
    return found


def test_every_operand_count_dtype_and_channel_count_is_instantiated(mine):
    assert set(one_trip(mine)) == {(t, k, c) for t in ("bf16_t", "f16_t") for k in range(1, 9) for c in (4, 8, 16)}


def test_no_scratch_and_no_flat_memory_operation(mine):
    for key, (lines, vgprs, scratch, private) in one_trip(mine).items():
        assert scratch == 0 and private == 0, (key, scratch, private)
        assert not any(l.startswith("flat_") for l in lines), key
        assert any(l.startswith("global_load_dwordx4") for l in lines) and any(l.startswith("global_store_dwordx4") for l in lines), key
        assert waves_per_simd(vgprs) == 8, (key, vgprs)  # the exchange's temporaries cost no wave


def test_the_exchange_costs_no_philox_multiply_and_the_register_table(mine, fast):
    "two whole blocks per lane, as in the contiguous kernel: no more 32 x 32 multiplies than its twin has"
    kernels = one_trip(mine)
    rows = []
    for t in ("bf16_t", "f16_t"):
        twin_lines, twin_vgprs, _, _ = next(body for name, body in fast.items() if TWIN.format(t=t) in name)
        which = tuple(w for w in WIDE_MUL if wide_multiplies(twin_lines, (w,)))  # whichever the twin compiles to
        assert which, t
        twin_muls = wide_multiplies(twin_lines, which)
        assert 30 <= twin_muls <= 40, twin_muls  # 2 blocks x 10 rounds x 2 products, less what constant folding takes
        for c in (4, 8, 16):
            lines, vgprs, _, _ = kernels[(t, 4, c)]
            muls = wide_multiplies(lines, WIDE_MUL)  # (every wide multiply of the kernel, in either spelling)
            rows.append(f"{t:7s} C={c:<2d} NumVgprs {vgprs:3d} (twin {twin_vgprs:3d})  wide multiplies {muls:2d} (twin {twin_muls:2d})  instructions {len(lines):3d} (twin {len(twin_lines):3d})")
            assert muls <= twin_muls, rows[-1]
    print("\n" + "\n".join(rows))


def test_the_exchange_runs_in_registers(mine):
    "DPP quad permutes for lane bits 0 and 1, ds_swizzle for bit 2; no LDS memory, no bpermute"
    for (t, k, c), (lines, _, _, _) in one_trip(mine).items():
        dpp = sum(1 for l in lines if "quad_perm" in l)
        swizzle = sum(1 for l in lines if l.startswith("ds_swizzle_b32"))
        assert not any(l.startswith(("ds_read", "ds_write", "ds_bpermute", "ds_permute")) for l in lines), (t, k, c)
        assert (dpp, swizzle) == EXCHANGE[c], (t, k, c, dpp, swizzle)
