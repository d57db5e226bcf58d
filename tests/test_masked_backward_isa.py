"""The one-trip masked backward kernel in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_masked_backward_launch` runs `masked_bwd_k1<T, KMAX>` (csrc/skr_step_masked_backward.hip) on launches of whole chunks.  What
the instruction stream shows of its contract: an instantiation per dtype and kernarg slot size, nothing spilled, global (not flat)
memory operations, the two loads (incoming gradient and mask) and a store per gradient slot.  The VGPR counts are printed for DESIGN.md
section 4.6; no occupancy bracket is asserted, and nothing else of the assembly is inspected."""

import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT

import __graft_entry__ as G

CSRC = os.path.join(ROOT, "skrample_amd", "csrc")
SOURCE = "skr_step_masked_backward.hip"
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SYMBOL = re.compile(r"masked_bwd_k1I(\w+?)Li(\d+)EE")
TYPES = {"bf16": "NS_6bf16_tE", "fp16": "NS_5f16_tE", "fp32": "f"}
SLOTS = (4, 8, 16)


def waves_per_simd(vgprs: int) -> int:
    "gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves"
    return min(8, 512 // (max(1, -(-vgprs // 8)) * 8))


def compiled(name: str, work: str) -> dict:
    "{symbol: (instructions and labels, VGPRs, scratch bytes, private segment size)} of every kernel of one source file"
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *G.PER_FILE_FLAGS.get(name, [])]
    os.makedirs(work)
    subprocess.run([HIPCC, *flags, "--save-temps", "-c", "-o", os.path.join(work, "x.o"), os.path.join(CSRC, name)], check=True, cwd=work, capture_output=True)
    asm = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(asm) == 1, asm
    text = open(os.path.join(work, asm[0])).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)", text, re.S | re.M):
        body = m.group(0).split(".Lfunc_end")[0]
        lines = [raw.split(";")[0].strip() for raw in body.splitlines()[1:]]
        private = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(0))
        out[m.group(1)] = ([l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))], int(m.group(2)), int(m.group(3)), int(private.group(1)) if private else None)
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    found = compiled(SOURCE, str(tmp_path_factory.mktemp("isa") / "masked_backward"))
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
