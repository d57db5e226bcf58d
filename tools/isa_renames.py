#!/usr/bin/env python3
"""The --renames map of tools/isa_compare.py for a refactor that respelled kernel templates without touching their code.

    python tools/isa_renames.py RULE WORK > MAP      (WORK: the --work directory of an isa_compare run over both trees)

Demangles the kernel symbols of both trees' assembly, rewrites each old template-id by the rule and prints one line
`OLD_SYMBOL NEW_SYMBOL` per old kernel the rule applies to; an old kernel whose new name no new symbol has is an error.  Rules:

  guided_forms  the six one-trip guided templates (guided[_rescaled]_kernel_v1<T, K, NOISE>, guided[_rescaled]_rows_kernel_v1<T, K, NOISE,
                RowForm>, guided[_rescaled]_rolling_kernel_v1<T, K, NOISE>) became guided_kernel_v1<T, K, NOISE, RowForm, RESCALE>, the two
                general kernels guided_kernel_gen<Acc, RESCALE>, and rescale_stats_{spans,final}_rows<T, PER_SAMPLE> /
                rescale_stats_{spans,final}_rolling<T> became rescale_stats_{spans,final}_rows<T, RowForm> (790 symbols)
  masked_forms  masked_kernel_v1<T, K, NOISE>, masked_rows_kernel_v1<T, K, NOISE, PER_SAMPLE> and masked_rolling_kernel_v1<T, K, NOISE>
                became masked_kernel_v1<T, K, NOISE, RowForm> (384 symbols)
  row_form      step_kernel_k1 / _rk1 / _k2 took the row form as a tag around the element type (PerSample<T>, Rolling<T>) and a bool
                TAB; they take RowForm where TAB stood (988 symbols: 328 Kernarg, 220 each WholeBatch, PerSample, Rolling)

RowForm (csrc/skr_step_common.h): Kernarg 0, WholeBatch 1, PerSample 2, Rolling 3."""

import glob
import re
import subprocess
import sys


def masked_forms(name: str, args: list[str]):
    if name == "masked_kernel_v1" and len(args) == 3:
        return name, args + ["(skr::RowForm)0"]
    if name == "masked_rows_kernel_v1":
        return "masked_kernel_v1", args[:3] + ["(skr::RowForm)2" if args[3] == "true" else "(skr::RowForm)1"]
    if name == "masked_rolling_kernel_v1":
        return "masked_kernel_v1", args + ["(skr::RowForm)3"]
    return None


def guided_forms(name: str, args: list[str]):
    step = re.fullmatch(r"guided_(rescaled_)?(rows_|rolling_)?kernel_(v1|gen)", name)
    if step and len(args) < (5 if step.group(3) == "v1" else 2):  # (a name of the new tree has its five, or two, arguments already)
        form = {None: ["(skr::RowForm)0"], "rows_": [], "rolling_": ["(skr::RowForm)3"]}[step.group(2)] if step.group(3) == "v1" else []
        return "guided_kernel_" + step.group(3), args + form + ["true" if step.group(1) else "false"]
    stats = re.fullmatch(r"rescale_stats_(spans|final)_(rows|rolling)", name)
    if stats and not args[-1].startswith("(skr::RowForm)"):
        form = 3 if stats.group(2) == "rolling" else 1 + (args[1] == "true")
        return f"rescale_stats_{stats.group(1)}_rows", [args[0], f"(skr::RowForm){form}"]
    return None


TAB_AT = {"step_kernel_k1": 5, "step_kernel_rk1": 4, "step_kernel_k2": 5}


def row_form(name: str, args: list[str]):
    if name not in TAB_AT:
        return None
    tag = re.fullmatch(r"skr::(PerSample|Rolling)<(.*)>", args[0])
    form = {"PerSample": 2, "Rolling": 3}[tag.group(1)] if tag else int(args[TAB_AT[name]] == "true")
    args = [tag.group(2) if tag else args[0], *args[1:]]
    args[TAB_AT[name]] = f"(skr::RowForm){form}"
    return name, args


RULES = {"guided_forms": guided_forms, "masked_forms": masked_forms, "row_form": row_form}


def template_ids(pattern: str) -> dict:
    "{demangled template-id, without the parameter list: symbol} of every kernel of the assembly files"
    symbols = sorted({s for path in glob.glob(pattern) for s in re.findall(r"^(_Z\w+):", open(path).read(), re.M)})
    names = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {name.rsplit(">(", 1)[0] + ">": symbol for symbol, name in zip(symbols, names) if ">(" in name}
    assert len(out) == sum(1 for name in names if ">(" in name), "two kernels of one template-id"
    return out


def main() -> int:
    rule, work = RULES[sys.argv[1]], sys.argv[2]
    new = template_ids(work + "/new/*.s")
    for old, symbol in template_ids(work + "/old/*.s").items():
        m = re.fullmatch(r"void skr::(\w+)<(.*)>", old)
        # (no template argument of these kernels holds a comma of its own)
        renamed = rule(m.group(1), m.group(2).split(", ")) if m else None
        if renamed:
            print(symbol, new[f"void skr::{renamed[0]}<{', '.join(renamed[1])}>"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
