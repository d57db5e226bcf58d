"""Channels-last step launches of two source trees timed side by side: a parent commit against this one, for a change that must not
move their speed (the shared draw exchange of csrc/skr_channels_last.h, the merged Python launchers and allocator).

  python tools/bench_channels_last_shared.py PARENT_TREE [NEW_TREE] [--repeats 5] [--steps 200] [--out profiles/channels_last_shared.txt]

Both trees are built already.  Every case is one child process of tools/bench_channels_last.py or tools/bench_masked_channels_last.py
(this tree's copies, `--tree` naming the package they time), the parent's child and the new tree's one after the other, case by case:
  forms a and c of both tools, both samplers   wall clock per step.  The masked form a prices the Python general path (evaluate_masked,
                                               the merged launcher and allocator); the plain forms ride the replayed fast path
  form k of the plain tool                     event clock per launch of step_kernel_cl1<bf16, 2, 8> and <bf16, 3, 16>: of the
                                               instantiations whose registers were renamed, the largest diff and the one extra s_waitcnt
Pass condition per case: the new median lies within the two runs' min - max spreads put together of the parent's median."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(tool, form, sampler, ()) for tool in ("bench_channels_last.py", "bench_masked_channels_last.py") for sampler in ("dpm2_sde", "dpm2") for form in ("a", "c")]
CASES += [("bench_channels_last.py", "k", "dpm2_sde", ("--operands", str(n), "--channels", str(c))) for n, c in ((2, 8), (3, 16))]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new", nargs="?", default=ROOT)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channels_last_shared.txt"))
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "new": os.path.abspath(args.new)}
    lines = [f"channels-last step launches, parent commit against this one: {args.repeats} repeats of {args.steps} steps per case, one child process per case and tree, parent and new alternating",
             "us per step (forms a, c: wall clock) or per launch (form k: event clock): median (min - max)"]  # fmt: skip
    failed = False
    for tool, form, sampler, extra in CASES:
        seen = {}
        for side, tree in trees.items():
            cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--repeats", str(args.repeats), "--steps", str(args.steps), "--tree", tree, *extra, "--child", form, sampler]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"{tool} form {form} / {sampler} of the {side} tree failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[side] = json.loads(found[-1][len("RESULT "):])
        if form == "k":
            name = f"step_kernel_cl1<bf16, {seen['new']['operands']}, {seen['new']['channels']}> alone"
            values = {side: seen[side]["cl1_us"] for side in trees}
        else:
            name = f"{'masked' if 'masked' in tool else 'plain '} form {form} {sampler}"
            values = {side: seen[side]["wall_us"] for side in trees}
            if seen["parent"]["checksum"] != seen["new"]["checksum"]:
                lines.append(f"  {name}: the two trees DISAGREE on the last result: {seen['parent']['checksum']!r} / {seen['new']['checksum']!r}")
                failed = True
        (pm, plo, phi), (nm, nlo, nhi) = ((statistics.median(v), min(v), max(v)) for v in (values["parent"], values["new"]))
        margin = (phi - plo) + (nhi - nlo)
        ok = abs(nm - pm) <= margin
        failed |= not ok
        lines.append(f"  {name:40s} parent {pm:8.2f} ({plo:8.2f} - {phi:8.2f})   new {nm:8.2f} ({nlo:8.2f} - {nhi:8.2f})   new - parent {nm - pm:+6.2f}, spreads together {margin:5.2f}: {'PASS' if ok else 'FAIL'}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
