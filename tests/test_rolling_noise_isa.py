"""The rolling forms of the Offset and Pyramid generator kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_noise_offset_rolling` and `skr_noise_pyramid_rolling` run `offset_kernel_v8<T, OffsetRollingArgs>`, the five
`pyramid_pass1<STRIP, THREADS, UNI, PyramidRollingArgs>` and `normalise_pass2<T, const int32_t*>` (csrc/skr_noise.hip): the whole-batch
kernels' own code behind one scalar load of the sample's index.  The contract is visible in the instruction stream, as that of the
rolling step kernels is (tests/test_masked_rolling_isa.py): a workgroup of an inactive sample ends on a scalar branch before its first
vector-memory instruction -- and before any LDS or Philox work, which the position of the branch shows -- no access is a flat one, and
no rolling kernel spills more than its whole-batch twin (the 1024-lane strips spill by design).  VGPR counts and waves per SIMD are
printed beside the twins' for DESIGN.md section 4.3; no occupancy bracket is asserted."""

import re

import pytest
from isa_cases import HIPCC, compile_asm, kernels_of, waves_per_simd

VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")
LDS = re.compile(r"^ds_")
BRANCH = ("s_cbranch_scc", "s_cbranch_vcc")
# (rolling symbol pattern, whole-batch twin pattern): the groups name the instantiation
FAMILIES = {
    "offset_kernel_v8": (re.compile(r"offset_kernel_v8I(\w+?)NS_17OffsetRollingArgsEEE"), re.compile(r"offset_kernel_v8I(\w+?)NS_10OffsetArgsEEE")),
    "pyramid_pass1": (re.compile(r"pyramid_pass1ILb([01])ELi(\d+)ELb([01])ENS_18PyramidRollingArgsEEE"), re.compile(r"pyramid_pass1ILb([01])ELi(\d+)ELb([01])ENS_11PyramidArgsEEE")),
    "normalise_pass2": (re.compile(r"normalise_pass2I(\w+?)JPKiEEE"), re.compile(r"normalise_pass2I(\w+?)JEEE")),
}
TYPES = {"DF16b", "DF16_", "f"}  # bf16, fp16, fp32: a rolling batch holds no fp64 latents
WANT = {
    "offset_kernel_v8": {(t,) for t in TYPES},
    "pyramid_pass1": {("0", "512", "0"), ("1", "256", "0"), ("1", "512", "0"), ("1", "1024", "0"), ("1", "1024", "1")},
    "normalise_pass2": {(t,) for t in TYPES},
}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    "{symbol: (instructions and labels, VGPRs, scratch bytes)} of every kernel of skr_noise.hip"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = kernels_of(compile_asm("skr_noise.hip", str(tmp_path_factory.mktemp("isa") / "noise")))
    return {k: v[:3] for k, v in found.items()}


@pytest.fixture(scope="module")
def pairs(compiled):
    "{(family, instantiation): (rolling kernel, whole-batch twin)}"
    found = {}
    for family, (rolling, twin) in FAMILIES.items():
        mine = {rolling.search(k).groups(): v for k, v in compiled.items() if rolling.search(k)}
        theirs = {twin.search(k).groups(): v for k, v in compiled.items() if twin.search(k)}
        assert set(mine) == WANT[family], (family, sorted(mine))
        for key, kernel in mine.items():
            assert key in theirs, (family, key)
            found[family, key] = (kernel, theirs[key])
    return found


def test_all_eleven_rolling_instantiations_exist(pairs):
    assert len(pairs) == 11


def test_inactive_exit_precedes_the_first_vector_memory_and_lds_instruction(pairs):
    "a conditional scalar branch whose target runs into s_endpgm, ahead of the first vector-memory and the first LDS instruction"
    for key, ((lines, *_), _) in pairs.items():
        first = min(i for i, l in enumerate(lines) if VMEM.match(l) or LDS.match(l))
        labels = {l[:-1]: i for i, l in enumerate(lines) if l.startswith(".LBB") and l.endswith(":")}
        exit_at = None
        for i, l in enumerate(lines[:first]):
            if exit_at is None and l.startswith(BRANCH):
                tail = [t for t in lines[labels[l.split()[-1]] :] if not t.startswith(".LBB")]
                if tail[0] == "s_endpgm":
                    exit_at = i
        assert exit_at is not None, (key, lines[:first][-12:])
        # the index itself came through the scalar cache, and no exec masking stands in for the branch
        assert any(l.startswith("s_load_dword ") for l in lines[:exit_at]), key
        assert not any("saveexec" in l for l in lines[:exit_at]), key


def test_no_flat_access(pairs):
    for key, ((lines, *_), _) in pairs.items():
        assert not any(l.startswith("flat_") for l in lines), key


def test_scratch_no_larger_than_the_twin(pairs):
    for key, ((_, _, scratch), (_, _, twin_scratch)) in pairs.items():
        assert scratch <= twin_scratch, (key, scratch, twin_scratch)


def test_vgpr_table_against_the_whole_batch_twins(pairs):
    "printed for DESIGN.md section 4.3 (run with -s); nothing is asserted: no occupancy bracket"
    print("\nVGPRs (waves per SIMD) / scratch bytes: rolling form vs whole-batch twin")
    for (family, key), ((_, vgprs, scratch), (_, twin_vgprs, twin_scratch)) in sorted(pairs.items()):
        print(f"  {family}<{', '.join(key)}>: {vgprs:3d} ({waves_per_simd(vgprs)}) / {scratch:4d}  vs  {twin_vgprs:3d} ({waves_per_simd(twin_vgprs)}) / {twin_scratch:4d}")
