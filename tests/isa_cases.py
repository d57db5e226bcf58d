"""What the ISA test modules share (no GPU needed: hipcc cross-compiles gfx950): one source file of skrample_amd/csrc compiled to
assembly with the library's own flags, the assembly split per kernel, occupancy from a VGPR count, demangled symbols, a file's
kernels by demangled name, the count of a Philox round's wide multiplies."""

from __future__ import annotations

import os
import re
import shutil
import subprocess

from conftest import ROOT

import __graft_entry__ as G

CSRC = os.path.join(ROOT, "skrample_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
CXXFILT = shutil.which("c++filt")
WIDE_MUL = ("v_mul_hi_u32", "v_mad_u64_u32")  # what a 32 x 32 -> 64 bit product of a Philox round compiles to
_asm: dict[str, str] = {}


def waves_per_simd(vgprs: int) -> int:
    "gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves"
    return min(8, 512 // (max(1, -(-vgprs // 8)) * 8))


def compile_asm(source_name: str, work: str) -> str:
    """the gfx950 assembly of csrc/<source_name>, compiled in the new directory `work` with the flags build() gives the file
    (--save-temps writes into the working directory of the compile, never into the tree); a file is compiled once per session"""
    if source_name not in _asm:
        flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *G.PER_FILE_FLAGS.get(source_name, [])]
        os.makedirs(work)
        subprocess.run([HIPCC, *flags, "--save-temps", "-c", "-o", os.path.join(work, "x.o"), os.path.join(CSRC, source_name)], check=True, cwd=work, capture_output=True)
        asm = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
        assert len(asm) == 1, asm
        with open(os.path.join(work, asm[0])) as fh:
            _asm[source_name] = fh.read()
    return _asm[source_name]


def kernels_of(text: str) -> dict:
    "{symbol: (instructions and .LBB labels, VGPRs, scratch bytes, private segment size)} of every kernel of an assembly text"
    private = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_private_segment_fixed_size (\d+)", text, re.S)}
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)", text, re.S | re.M):
        body = m.group(0).split(".Lfunc_end")[0]
        lines = [raw.split(";")[0].strip() for raw in body.splitlines()[1:]]  # (comments: `;` to the end of the line)
        out[m.group(1)] = ([l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))], int(m.group(2)), int(m.group(3)), private.get(m.group(1)))
    return out


def demangle(symbols) -> dict:
    """{symbol: demangled name}, through c++filt (`DF16b`, __bf16, is newer than GNU's demangler: given the vendor-type spelling it
    understands, as tools/kernel_stats.py does); a symbol it does not know comes back as it went in"""
    symbols = list(symbols)
    out = subprocess.run([CXXFILT], input="\n".join(s.replace("DF16b", "u6__bf16") for s in symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    return {s: (name if name and not name.startswith("_Z") else s) for s, name in zip(symbols, out)}


def named(source, work):
    "{demangled name: kernels_of's entry} of every kernel of csrc/<source>"
    kernels = kernels_of(compile_asm(source, work))
    names = demangle(kernels)
    return {names[sym]: body for sym, body in kernels.items()}


def wide_multiplies(lines, which):
    return sum(1 for l in lines if l.split()[0] in which)
