"""The per-sample step kernels in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

`skr_step_launch_indexed_per_sample` runs per-sample forms of the table (`TAB`) instantiations of the one-trip kernels
(csrc/skr_step_fast.hip: step_kernel_k1 / _k2 / _rk1 with the element type wrapped in `PerSample<>`).  A workgroup belongs to one
sample, so the per-sample index and the row it names must be fetched by scalar loads, exactly as the whole-batch form fetches
`index[0]` and its row -- as per-lane vector loads they would add vector-memory traffic to an HBM-bound kernel.  This module compiles
the file with the library's own flags and compares every per-sample instantiation with its whole-batch twin: no more vector-memory
loads, no scratch, the same occupancy."""

import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT

import __graft_entry__ as G

SRC = os.path.join(ROOT, "skrample_amd", "csrc", "skr_step_fast.hip")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
VLOAD = re.compile(r"^(global|flat|buffer|scratch)_load")
SLOAD = re.compile(r"^s_(buffer_)?load")
TAG = re.compile(r"NS_9PerSampleI(.*?)EE")  # the mangled PerSample<T> wrapper around the element type


def waves_per_simd(vgprs: int) -> int:
    "gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves"
    return min(8, 512 // (max(1, -(-vgprs // 8)) * 8))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    "{symbol: (instructions, VGPRs, scratch bytes, private segment size)} of every kernel of skr_step_fast.hip"
    if HIPCC is None:
        pytest.skip("no hipcc on this box")
    work = str(tmp_path_factory.mktemp("isa"))
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *G.PER_FILE_FLAGS.get(os.path.basename(SRC), [])]
    subprocess.run([HIPCC, *flags, "--save-temps", "-c", "-o", os.path.join(work, "x.o"), SRC], check=True, cwd=work, capture_output=True)
    asm = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(asm) == 1, asm
    text = open(os.path.join(work, asm[0])).read()
    private = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S)}
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)", text, re.S | re.M):
        body = m.group(0).split(".Lfunc_end")[0]
        lines = [raw.split(";")[0].strip() for raw in body.splitlines()[1:]]
        out[m.group(1)] = ([l for l in lines if l and not l.startswith(".")], int(m.group(2)), int(m.group(3)), private[m.group(1)])
    return out


def pairs(kernels):
    found = [(k, TAG.sub(r"\1", k, count=1)) for k in kernels if "PerSample" in k]
    for k, twin in found:
        assert twin in kernels, ("no whole-batch twin", k)
    return found


def test_every_table_instantiation_has_a_per_sample_form(kernels):
    "the TAB (last-but-BLK / last bool = true) instantiations of the three kernels, and their per-sample forms, one to one"
    found = pairs(kernels)
    for name in ("step_kernel_k1I", "step_kernel_k2I", "step_kernel_rk1I"):
        assert sum(1 for k, _ in found if name in k) >= 20, name
    tabs = set()
    for k in kernels:
        if "PerSample" in k:
            continue
        if re.search(r"14step_kernel_k1I.*Lb1EEEvNS_11OneTripArgs", k) or re.search(r"15step_kernel_rk1I.*Lb1ELi\d+EEEvNS_13RkOneTripArgs", k) or re.search(r"14step_kernel_k2I.*Lb1ELb0EEEvNS_10TwoOutArgs", k):
            tabs.add(k)
    assert tabs == {twin for _, twin in found}, sorted(tabs ^ {twin for _, twin in found})[:4]


def test_row_and_index_fetches_stay_scalar(kernels):
    "(a) no per-sample instantiation has more vector-memory loads than its twin; the index and row fetches show up as scalar loads"
    for k, twin in pairs(kernels):
        mine, theirs = kernels[k][0], kernels[twin][0]
        count = lambda lines, what: sum(1 for l in lines if what.match(l))  # noqa: E731
        assert count(mine, VLOAD) <= count(theirs, VLOAD), (k, count(mine, VLOAD), count(theirs, VLOAD))
        assert count(mine, SLOAD) >= 3, k  # kernarg, index entry, row
        assert any(l.startswith("v_readfirstlane") for l in mine), k  # the sample id of the dividing chunk -> sample map


def test_no_scratch_and_the_twins_occupancy(kernels):
    "(b) private segment size 0, and the VGPR count in the occupancy bracket of the twin"
    for k, twin in pairs(kernels):
        _, vgprs, scratch, private = kernels[k]
        assert scratch == 0 and private == 0, (k, scratch, private)
        assert waves_per_simd(vgprs) >= waves_per_simd(kernels[twin][1]), (k, vgprs, kernels[twin][1])
