#!/usr/bin/env python3
"""The --renames map of tools/isa_compare.py for the merge of the three one-trip masked kernel templates into one.

    python tools/masked_forms_renames.py WORK > MAP      (WORK: the --work directory of an isa_compare run over both trees)

masked_kernel_v1<T, K, NOISE>, masked_rows_kernel_v1<T, K, NOISE, PER_SAMPLE> and masked_rolling_kernel_v1<T, K, NOISE> of the old tree are
masked_kernel_v1<T, K, NOISE, RowForm> of the new one, with RowForm Kernarg 0, WholeBatch 1, PerSample 2, Rolling 3.  Prints one line
`OLD_SYMBOL NEW_SYMBOL` per old kernel, read off the two trees' assembly."""

import glob
import re
import sys

OLD = (
    (re.compile(r"^(_ZN3skr16masked_kernel_v1I(\w+?)Li(\d+)ELb([01])EE\w*):", re.M), lambda m: "0"),
    (re.compile(r"^(_ZN3skr21masked_rows_kernel_v1I(\w+?)Li(\d+)ELb([01])ELb([01])EE\w*):", re.M), lambda m: "12"[int(m.group(5))]),
    (re.compile(r"^(_ZN3skr24masked_rolling_kernel_v1I(\w+?)Li(\d+)ELb([01])EE\w*):", re.M), lambda m: "3"),
)
NEW = re.compile(r"^(_ZN3skr16masked_kernel_v1I(\w+?)Li(\d+)ELb([01])ELNS_7RowFormE([0-3])EE\w*):", re.M)


def main() -> int:
    work = sys.argv[1]
    new = {m.groups()[1:]: m.group(1) for path in glob.glob(work + "/new/skr_step_masked*.s") for m in NEW.finditer(open(path).read())}
    for path in sorted(glob.glob(work + "/old/skr_step_masked*.s")):
        text = open(path).read()
        for pattern, form in OLD:
            for m in pattern.finditer(text):
                print(m.group(1), new[(*m.groups()[1:4], form(m))])
    return 0


if __name__ == "__main__":
    sys.exit(main())
