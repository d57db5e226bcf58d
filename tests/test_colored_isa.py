"""The plane claim of colored_inverse128 in the compiled ISA (no GPU needed: hipcc cross-compiles gfx950).

The persistent inverse kernel claims the plane of the trip after next with a returning atomic written as inline assembly, and waits
for it with an inline `s_waitcnt vmcnt(17)` after the prefetch (csrc/skr_colored.hip, colored_inverse128).  The compiler does not know
the atomic is in flight, so the claim is only correct while the code it emits around it keeps three properties: nothing touches the
atomic's destination register before the wait, at least 17 vector-memory instructions are issued behind the atomic on every way to the
wait (else vmcnt(17) does not imply that the atomic has returned), and the claimed value is first read after the wait.  This module
compiles the file with the library's own flags and checks the three on every path of the control-flow graph between the two, for
each output type -- so that a compiler version that copies, spills or reorders the register fails here and not on the device."""

import heapq
import re

import pytest
from isa_cases import HIPCC, compile_asm

KERNELS = {"DF16b": "bf16", "DF16_": "f16", "f": "f32"}  # mangled template argument of colored_inverse128<T>
WAIT = "s_waitcnt vmcnt(17)"
VMEM = ("global_", "buffer_", "flat_", "scratch_")  # every instruction vmcnt counts on gfx950 (loads, stores and atomics)
BRANCH = re.compile(r"s_(c?branch\w*)\s+(\S+)")
VMCNT = re.compile(r"s_waitcnt\b.*\bvmcnt\((\d+)\)")


def inverse128_kernels(text: str) -> dict[str, list[str]]:
    "{bf16 / f16 / f32: the kernel's instruction and label lines} cut from the assembly (tools/isa_mix.py's cut, to the function's end)"
    out = {}
    for m in re.finditer(r"^(_ZN3skr18colored_inverse128I(\w+?)EEvNS_11ColoredArgsEl):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        assert m.group(2) in KERNELS, m.group(1)
        lines = []
        for raw in m.group(0).splitlines()[1:-1]:
            line = raw.split(";")[0].strip()  # (comments: `;` to the end of the line)
            if line and not line.startswith("."):
                lines.append(line)
            elif re.match(r"^\.LBB\w+:", line):
                lines.append(line)
        out[KERNELS[m.group(2)]] = lines
    return out


def vgprs(operands: str) -> set[int]:
    "the VGPR numbers an operand list names (v7, v[4:7])"
    regs = {int(r) for r in re.findall(r"(?<![\w\[])v(\d+)\b", operands)}
    for lo, hi in re.findall(r"(?<!\w)v\[(\d+):(\d+)\]", operands):
        regs.update(range(int(lo), int(hi) + 1))
    return regs


def split(line: str) -> tuple[str, str]:
    op, _, rest = line.partition(" ")
    return op, rest


def reads(line: str) -> set[int]:
    "VGPRs an instruction reads: every operand of a store / write / non-returning atomic, all but the first of anything else"
    op, rest = split(line)
    if op.startswith(("s_", ".")):
        return set()
    stores = op.startswith(("global_store", "buffer_store", "flat_store", "scratch_store")) or (op.startswith("ds_") and "read" not in op and "_rtn" not in op)
    stores |= "atomic" in op and not re.search(r"\b(sc0|glc)\b", rest)
    if stores:
        return vgprs(rest)
    return vgprs(rest.partition(",")[2])


def touches(line: str) -> set[int]:
    op, rest = split(line)
    return set() if op.startswith(".") else vgprs(rest)


class CFG:
    "control flow between the lines of one kernel: a block starts at a label or after a branch, and ends at a branch or before the next label"

    def __init__(self, lines: list[str]):
        self.lines = lines
        start = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
        self.next: list[list[int]] = []
        for i, l in enumerate(lines):
            m = BRANCH.match(l)
            if l.startswith(("s_endpgm", "s_setpc", "s_trap")):
                self.next.append([])
            elif m and m.group(1) == "branch":
                self.next.append([start[m.group(2)]])
            else:
                self.next.append(([i + 1] if i + 1 < len(lines) else []) + ([start[m.group(2)]] if m else []))
        self.prev: list[list[int]] = [[] for _ in lines]
        for i, succ in enumerate(self.next):
            for j in succ:
                self.prev[j].append(i)

    def forward(self, i: int, stop: set[int]) -> dict[int, int]:
        """every line reachable from line i (i itself only by a cycle) while the vector-memory instruction at line i may still be in
        flight, with the fewest vector-memory instructions issued after line i on the way to it.  A path ends at a line of `stop` and at
        an `s_waitcnt vmcnt(N)` that at least N younger instructions on it make sure of (those lines are reached but not passed)."""
        best: dict[int, int] = {}
        heap = [(0, j) for j in self.next[i]]
        while heap:
            n, j = heapq.heappop(heap)
            if j in best:
                continue
            best[j] = n
            wait = VMCNT.match(self.lines[j])
            if j in stop or (wait and n >= int(wait.group(1))):
                continue
            n += self.lines[j].startswith(VMEM)
            for k in self.next[j]:
                heapq.heappush(heap, (n, k))
        return best

    def backward(self, i: int, within: set[int]) -> set[int]:
        "every line of `within` from which line i is reachable through lines of `within`"
        seen, todo = set(), list(self.prev[i])
        while todo:
            j = todo.pop()
            if j in seen or j not in within:
                continue
            seen.add(j)
            todo.extend(self.prev[j])
        return seen


def check_claim(lines: list[str]) -> dict:
    "the conditions of the claim in one kernel; returns what was measured (asserts on a violation)"
    atomics = [i for i, l in enumerate(lines) if l.startswith("global_atomic_add") and re.search(r"\bsc0\b", l)]
    assert len(atomics) == 1, ("one returning global_atomic_add per kernel", [lines[i] for i in atomics])
    at = atomics[0]
    dst = vgprs(split(lines[at])[1].partition(",")[0])
    assert len(dst) == 1, lines[at]
    waits = [i for i, l in enumerate(lines) if l == WAIT]
    assert len(waits) == 1, ("one " + WAIT + " per kernel", len(waits))
    wait = waits[0]
    cfg = CFG(lines)
    fwd = cfg.forward(at, {wait, at})
    assert wait in fwd, "the wait is not reachable from the atomic"
    # the lines on some path from the atomic to the wait along which the atomic may be in flight (a path around the loop that meets
    # an earlier wait sufficient for it ends there)
    between = sorted(cfg.backward(wait, {j for j in fwd if j not in (wait, at) and not (VMCNT.match(lines[j]) and fwd[j] >= int(VMCNT.match(lines[j]).group(1)))}))
    # nothing on any of those paths reads or writes the atomic's destination
    bad = [(j, lines[j]) for j in between if touches(lines[j]) & dst]
    assert not bad, ("the atomic's destination is used before the wait", bad)
    # every path issues at least 17 vector-memory instructions behind the atomic: vmcnt(17) then implies the atomic has returned
    assert fwd[wait] >= 17, "a path from the atomic to the wait issues only %d vector-memory instructions" % fwd[wait]
    # the claimed value is first read after the wait
    first_read = next((j for j in range(at + 1, len(lines)) if reads(lines[j]) & dst), None)
    assert first_read is not None and first_read > wait, ("first read of the claimed register", first_read, wait)
    return {"dst": sorted(dst), "min_vmem": fwd[wait], "between": len(between), "branches": sum(1 for j in between if BRANCH.match(lines[j]))}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    found = inverse128_kernels(compile_asm("skr_colored.hip", str(tmp_path_factory.mktemp("isa") / "colored")))
    assert sorted(found) == sorted(KERNELS.values()), sorted(found)
    return found


@pytest.mark.parametrize("dtype", sorted(KERNELS.values()))
def test_inverse128_plane_claim_is_waited_for(kernels, dtype):
    got = check_claim(kernels[dtype])
    assert got["min_vmem"] >= 17 and got["branches"] >= 1, got  # (the window holds branches: a text-order check alone would not do)


def test_the_claim_check_fails_on_broken_code():
    "the checker itself, on hand-written kernels: a use of the register, too few loads on one path, no wait, an early read"
    loads = ["global_load_dwordx2 v[%d:%d], v[4:5], off" % (10 + 2 * k, 11 + 2 * k) for k in range(17)]
    good = ["v_mov_b32_e32 v0, 0", "global_atomic_add v0, v33, v86, s[14:15] sc0", "s_cbranch_vccnz .LBB0_2", *loads, ".LBB0_2:", *loads, WAIT, "ds_write_b32 v33, v0", "s_endpgm"]
    # (both ways issue 17 loads: the branch skips the first group, the second one is on both)
    assert check_claim(good)["min_vmem"] == 17
    broken = {
        "register used": good[:5] + ["v_mov_b32_e32 v1, v0"] + good[5:],
        "too few loads on one path": good[:3] + loads + [".LBB0_2:"] + loads[1:] + good[3 + 17 + 1 + 17 :],
        "no wait": [l for l in good if l != WAIT],
        "wait moved above the loads": good[:3] + [WAIT] + [l for l in good[3:] if l != WAIT],
        "read before the wait": good[:-3] + ["v_readfirstlane_b32 s0, v0", WAIT] + good[-2:],
    }
    for lines in broken.values():
        with pytest.raises(AssertionError):
            check_claim(lines)
