#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel symbol by kernel symbol (no GPU needed).

    python tools/isa_compare.py OLD_TREE NEW_TREE [--files NAME.hip ...] [--jobs N] [--work DIR] [--renames FILE] [--pooled] [--classify]

Compiles the named files of skrample_amd/csrc (default: the step files skr_step.hip, skr_step_fast.hip, skr_step_backward.hip and
skr_tape.hip) of each tree with the library's own flags, the tree's PER_FILE_FLAGS included (`--save-temps -c`), splits the device assembly per kernel the way tests/isa_cases.py does,
and reports symbols found in one tree only and, for each common symbol, whether its instruction lines (comments stripped, labels
kept, numbered within their kernel), TotalNumSgprs, NumVgprs, ScratchSize or its `.amdhsa_*` descriptor lines differ, with a unified
diff per differing symbol.
A host-side refactor must end in `0 added, 0 removed, 0 differing` for every file.  Exit status 1 when anything differs.
With --work DIR the assembly is kept there and reused while it is newer than the tree's sources.
With --renames FILE (lines of `OLD_SYMBOL NEW_SYMBOL`, written by hand or by tools/isa_renames.py: a kernel template that gained a parameter) an old kernel is compared under its new
name; the map is printed ahead of the report (its size alone when it is long).
With --pooled (kernels that moved between files, files merged or split) the kernels of all named files of a tree are pooled and the two
pools compared; a named file may then be missing from either tree, and a symbol defined twice in one pool is an error.
With --classify (a device-side refactor that may only reorder) every differing symbol is named `reordered only` -- the same NumVgprs,
TotalNumSgprs and ScratchSize, the same `.amdhsa_*` lines and, with s_waitcnt and s_nop set aside, the same multiset of opcodes -- or
by the first of these it fails, and the exit status is 0 when every difference is of the first kind."""

from __future__ import annotations

import argparse
import collections
import difflib
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FILES = ("skr_step.hip", "skr_step_fast.hip", "skr_step_backward.hip", "skr_tape.hip")
KERNEL = re.compile(r"^(_Z\w+):.*?^\.Lfunc_end\d+:.*?; TotalNumSgprs: (\d+).*?; NumVgprs: (\d+).*?; ScratchSize: (\d+)", re.S | re.M)


def per_file_flags(tree: str) -> dict:
    spec = importlib.util.spec_from_file_location("_entry_of_tree", os.path.join(tree, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PER_FILE_FLAGS


def assembly(tree: str, name: str, work: str, hipcc: str) -> str:
    "device assembly of one source file of one tree"
    out = os.path.join(work, name + ".s")
    deps = glob.glob(os.path.join(tree, "skrample_amd", "csrc", "*.h*")) + [os.path.join(tree, "include", "skrample_hip.h")]
    if os.path.isfile(out) and os.path.getmtime(out) > max(os.path.getmtime(p) for p in deps):
        return open(out).read()
    tmp = os.path.join(work, name + ".tmp")
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(tmp)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *per_file_flags(tree).get(name, [])]
    subprocess.run([hipcc, *flags, "--save-temps", "-c", "-o", os.path.join(tmp, "x.o"), os.path.join(tree, "skrample_amd", "csrc", name)], check=True, cwd=tmp)
    asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
    assert len(asm) == 1, asm
    os.replace(os.path.join(tmp, asm[0]), out)
    shutil.rmtree(tmp)
    return open(out).read()


def kernels(text: str) -> dict:
    "{symbol: lines to compare}: instructions and labels, then the register / scratch figures, then the kernel descriptor"
    out = {}
    for m in KERNEL.finditer(text):
        body = m.group(0).split(".Lfunc_end")[0]
        # (a block label carries the function's position in the file, `.LBB<function>_<block>`: dropped, so that the order in which
        #  the kernels are emitted does not count)
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", raw.split(";")[0].strip()) for raw in body.splitlines()[1:]]
        code = [l for l in lines if l and (not l.startswith(".") or l.startswith(".LBB"))]
        figures = [f"; TotalNumSgprs: {m.group(2)}", f"; NumVgprs: {m.group(3)}", f"; ScratchSize: {m.group(4)}"]
        out[m.group(1)] = code + figures + [l for l in lines if l.startswith(".amdhsa_")]
    return out


def verdict(old: list, new: list) -> str:
    "`reordered only`, or the first criterion a differing symbol fails (--classify)"

    def part(lines, keep):
        return [l for l in lines if keep(l)]

    for what, keep in (("register / scratch figures", lambda l: l.startswith("; ")), (".amdhsa_ lines", lambda l: l.startswith(".amdhsa_"))):
        if part(old, keep) != part(new, keep):
            return what + " differ"

    def opcodes(lines):
        code = part(lines, lambda l: not l.startswith((";", ".")) and not l.endswith(":"))
        return collections.Counter(op for op in (l.split()[0] for l in code) if op not in ("s_waitcnt", "s_nop"))

    a, b = opcodes(old), opcodes(new)
    if a != b:
        return "opcode multiset differs: " + ", ".join(f"{op} {a[op]} -> {b[op]}" for op in sorted(set(a) | set(b)) if a[op] != b[op])
    return "reordered only"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--files", nargs="+", default=list(FILES), metavar="NAME.hip", help="sources of skrample_amd/csrc to compare (default: the four step files)")
    ap.add_argument("--jobs", type=int, default=8, help="compilations at a time (at most 16)")
    ap.add_argument("--work", default=None, help="directory that keeps the assembly between runs")
    ap.add_argument("--renames", default=None, metavar="FILE", help="lines of `OLD_SYMBOL NEW_SYMBOL`: old kernels compared under their new names")
    ap.add_argument("--pooled", action="store_true", help="compare the union of the kernels of the named files of each tree (a file may be missing from one)")
    ap.add_argument("--classify", action="store_true", help="name each differing symbol `reordered only` or the criterion it fails; exit 0 when all are the former")
    a = ap.parse_args()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    work = a.work or tempfile.mkdtemp(prefix="isa_compare_")
    trees = {"old": os.path.abspath(a.old), "new": os.path.abspath(a.new)}
    for side in trees:
        os.makedirs(os.path.join(work, side), exist_ok=True)
    jobs = [(side, name) for name in a.files for side in trees if not a.pooled or os.path.isfile(os.path.join(trees[side], "skrample_amd", "csrc", name))]
    with ThreadPoolExecutor(max_workers=max(1, min(16, a.jobs))) as pool:
        texts = dict(zip(jobs, pool.map(lambda j: assembly(trees[j[0]], j[1], os.path.join(work, j[0]), hipcc), jobs)))
    renames = dict(line.split() for line in open(a.renames) if line.strip()) if a.renames else {}
    if len(renames) > 16:
        print(f"renamed: {len(renames)} symbols ({a.renames})")
    else:
        for was, now in renames.items():
            print(f"renamed: {was} -> {now}")

    def pooled(side: str) -> dict:
        "the kernels of every named file that the tree has"
        out, census = {}, []
        for name in a.files:
            found = kernels(texts[side, name]) if (side, name) in texts else None
            census.append(f"{name} absent" if found is None else f"{name} {len(found)}")
            assert not set(found or ()) & set(out), (side, name, sorted(set(found) & set(out))[:3])
            out.update(found or {})
        print(f"{side}: " + ", ".join(census))
        return out

    bad = 0
    for name in ["pooled"] if a.pooled else a.files:
        old, new = (pooled("old"), pooled("new")) if a.pooled else (kernels(texts["old", name]), kernels(texts["new", name]))
        old = {renames.get(k, k): [l.replace(k, renames[k]) for l in v] if k in renames else v for k, v in old.items()}
        added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
        differing = [k for k in sorted(set(old) & set(new)) if old[k] != new[k]]
        for k in differing:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(old[k], new[k], "old/" + k, "new/" + k, lineterm=""))
        for k in added:
            print(f"only in new: {k}")
        for k in removed:
            print(f"only in old: {k}")
        print(f"{name}: {len(old)} kernels old, {len(new)} new: {len(added)} added, {len(removed)} removed, {len(differing)} differing")
        if a.classify:
            verdicts = {k: verdict(old[k], new[k]) for k in differing}
            for k in differing:
                print(f"{k}: {verdicts[k]}")
            differing = [k for k in differing if verdicts[k] != "reordered only"]
        bad += len(added) + len(removed) + len(differing)
    if a.work is None:
        shutil.rmtree(work)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
