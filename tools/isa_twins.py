#!/usr/bin/env python3
"""VGPRs, scratch and waves per SIMD of every *_rolling_kernel_v1 beside its PerSample twin (no GPU needed).

    python tools/isa_twins.py WORK/new/skr_step_thresholded_rows.hip.s
    python tools/isa_twins.py WORK/new/skr_step_projected_rolling.hip.s WORK/new/skr_step_projected_rows.hip.s

The arguments are the device assembly that `tools/isa_compare.py OLD NEW --files ... --work WORK` keeps: one file where the rolling kernel
and its twin share a translation unit, the rolling kernel's and the twin's where they do not.  The figures are the compiler's own; an
instantiation below its twin's occupancy is marked."""

import re
import sys

KERNEL = re.compile(r"^(_Z\w+):.*?^\.Lfunc_end\d+:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", re.S | re.M)
DTYPE = {"NS_5f16_tE": "fp16", "NS_6bf16_tE": "bf16", "f": "fp32"}


def main() -> int:
    rolling, twin = {}, {}
    for m in KERNEL.finditer("\n".join(open(path).read() for path in sys.argv[1:])):
        k = re.search(r"kernel_v1I(NS_5f16_tE|NS_6bf16_tE|f)Li(\d+)ELb(\d)", m.group(1))
        if k is None:
            continue
        key = (DTYPE[k.group(1)], int(k.group(2)), int(k.group(3)))
        if "_rolling_kernel" in m.group(1):
            rolling[key] = m.groups()[1:]
        elif "RowFormE2" in m.group(1):  # RowForm::PerSample
            twin[key] = m.groups()[1:]
    below = 0
    print("dtype  K noise | Rolling VGPRs scratch waves/SIMD | PerSample VGPRs scratch waves/SIMD")
    for key in sorted(rolling):
        r, p = rolling[key], twin[key]
        lost = int(r[2]) < int(p[2])
        below += lost
        print(f"{key[0]:5s} {key[1]:2d} {key[2]}     | {r[0]:>4s} {r[1]:>3s} {r[2]:>2s} | {p[0]:>4s} {p[1]:>3s} {p[2]:>2s}" + ("   <- one bracket below its twin" if lost else ""))
    print(f"{len(rolling)} Rolling instantiations, {sum(int(r[1]) > 0 for r in rolling.values())} with scratch, {below} below their twin's occupancy")
    return 0


if __name__ == "__main__":
    sys.exit(main())
