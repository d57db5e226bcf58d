"""The one-trip masked backward kernel in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_masked_backward_launch` runs `masked_bwd_k1<T, KMAX>` (csrc/skr_step_backward.hip) on launches of whole chunks.  What
the instruction stream shows of its contract: an instantiation per dtype and kernarg slot size, nothing spilled, global (not flat)
memory operations, the two loads (incoming gradient and mask) and a store per gradient slot.  The VGPR counts are printed for DESIGN.md
section 4.6; no occupancy bracket is asserted, and nothing else of the assembly is inspected."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

SOURCE = "skr_step_backward.hip"
SYMBOL = re.compile(r"masked_bwd_k1I(\w+?)Li(\d+)EE")
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}
SLOTS = (4, 8, 16)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm(SOURCE, str(tmp_path_factory.mktemp("isa") / "backward")))
    return {SYMBOL.search(k).groups(): v for k, v in found.items() if SYMBOL.search(k)}


def test_an_instantiation_for_every_dtype_and_slot_size(kernels):
    want = {(t, str(n)) for t in TYPES.values() for n in SLOTS}
    assert set(kernels) == want, (sorted(want - set(kernels)), sorted(set(kernels) - want))


def test_no_scratch(kernels):
    for key, (lines, _, scratch, private) in kernels.items():
        assert scratch == 0 and private == 0, (key, scratch, private)
        assert not any(l.startswith("scratch_") for l in lines), key


def test_memory_operations_are_global(kernels):
    "no flat access; the incoming gradient and the mask are loaded, and every gradient slot is stored"
    for key, (lines, *_) in kernels.items():
        assert not any(l.startswith("flat_") for l in lines), key
        assert sum(1 for l in lines if l.startswith("global_load")) >= 2, key
        assert sum(1 for l in lines if l.startswith("global_store")) >= int(key[1]), key


def test_vgpr_table(kernels):
    "printed for DESIGN.md section 4.6 (run with -s); nothing is asserted of the counts"
    names = {v: k for k, v in TYPES.items()}
    print("\nVGPRs (waves per SIMD) of masked_bwd_k1<T, KMAX>")
    for key in sorted(kernels, key=lambda g: (g[0], int(g[1]))):
        vgprs = kernels[key][1]
        print(f"  {names[key[0]]} KMAX={int(key[1]):2d}: {vgprs:3d} ({waves_per_simd(vgprs)})")
