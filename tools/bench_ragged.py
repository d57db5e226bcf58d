"""Cost of a rolling step launch on ragged samples against its whole-chunk twin and against what a user had before, through the C ABI:
skr_step_launch_rolling with 4 bf16 operands and in-kernel noise, capacity 64, every slot active.

  python tools/bench_ragged.py [--repeats 7] [--launches 2000] [--out profiles/ragged_samples.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  r  ragged     64 x (4, 144, 112): 31.5 chunks a sample, step_kernel_ragged (csrc/skr_step_ragged.hip) -- the new form
  w  whole      64 x (4, 128, 128): 32 chunks a sample, step_kernel_k1 (csrc/skr_step_fast.hip) -- the twin, untouched code
  e  eager x64  what (4, 144, 112) requests had before: 64 skr_step_launch calls of one sample each, every one with its own plan
Per repeat, `launches` launches (form e: `launches` rounds of 64 calls) are timed with HIP events (first enqueue to last kernel) after a
warm-up of 100; reported per form: median and min - max over the repeats, us per launch, and for r and w us per algorithmic MB -- the
bytes the step must move, (4 operands + 1 output) x elements x 2 bytes.
The expectation is written ahead of the run, at the head of the report; behind the numbers stands whether it held."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, OPERANDS, WARMUP = 64, 4, 100
SHAPES = {"r": (4, 144, 112), "w": (4, 128, 128), "e": (4, 144, 112)}
FORMS = {"r": "rolling, ragged 64 x (4,144,112)", "w": "rolling, whole 64 x (4,128,128)", "e": "64 eager launches of (4,144,112)"}
EXPECTATION = (
    "expectation (written before the run): per algorithmic byte the ragged form lies above its whole-chunk twin by no more than the half-empty\n"
    "last chunk of every sample -- 32 workgroups for 31.5 chunks of data, 1.6 % -- plus the two forms' min - max spreads together."
)


def algorithmic_mb(form: str) -> float:
    c, h, w = SHAPES[form]
    return (OPERANDS + 1) * CAPACITY * c * h * w * 2 / 1e6


def child(form: str, repeats: int, launches: int) -> None:
    import torch

    from skrample_amd import _hip

    dev = torch.device("cuda:0")
    lib, stream = _hip.load(), _hip.current_stream_ptr(dev)
    c, h, w = SHAPES[form]
    sample = c * h * w
    numel = CAPACITY * sample
    g = torch.Generator().manual_seed(1)
    ops = [torch.randn(numel, generator=g).bfloat16().to(dev) for _ in range(OPERANDS)]
    out = torch.empty(numel, dtype=torch.bfloat16, device=dev)
    seeds = torch.arange(1, CAPACITY + 1, dtype=torch.int64, device=dev)
    code = _hip.DTYPE_CODE[torch.bfloat16]

    def plan_of(b: int) -> "_hip.StepPlanC":
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = OPERANDS
        plan.dtype_a = plan.dtype_b = plan.out0_dtype = code
        plan.out1_dtype, plan.noise_mode, plan.sample_numel = _hip.NONE, 1, sample
        for k in range(OPERANDS):
            plan.coef0[k] = 0.25 * (k + 1) * (-1) ** (k + b)
        plan.zeta0, plan.stream0 = 0.5 + b / 256, 256 * b
        return plan

    plans = [plan_of(b) for b in range(CAPACITY)]
    if form == "e":
        parts = [(ctypes.c_void_p * OPERANDS)(*[t[b * sample : (b + 1) * sample].data_ptr() for t in ops]) for b in range(CAPACITY)]
        outs = [out[b * sample : (b + 1) * sample].data_ptr() for b in range(CAPACITY)]
        seed_ptrs = [seeds[b : b + 1].data_ptr() for b in range(CAPACITY)]
        refs = [ctypes.byref(p) for p in plans]

        def launch() -> int:
            status = 0
            for b in range(CAPACITY):
                status |= lib.skr_step_launch(refs[b], parts[b], outs[b], None, seed_ptrs[b], sample, stream)
            return status
    else:
        rows = (_hip.StepRowC * CAPACITY)(*[_hip.IndexedRows.row_from(p) for p in plans])  # every slot at a row of its own
        rows_dev = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
        index = torch.arange(CAPACITY, dtype=torch.int32, device=dev)
        ptrs = (ctypes.c_void_p * OPERANDS)(*[t.data_ptr() for t in ops])
        plan = ctypes.byref(plans[0])
        fixed = (ptrs, out.data_ptr(), None, seeds.data_ptr(), numel, rows_dev.data_ptr(), index.data_ptr(), 0, stream)

        def launch() -> int:
            return lib.skr_step_launch_rolling(plan, *fixed)

    for _ in range(WARMUP):
        _hip.check(launch(), "launch")
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = 0
        for _ in range(launches):
            status |= launch()
        e1.record()
        torch.cuda.synchronize()
        _hip.check(status, "launch")
        event_us.append(e0.elapsed_time(e1) * 1e3 / launches)
    assert torch.isfinite(out.float()).all()
    print("RESULT " + json.dumps({"form": form, "event_us": event_us, "device": torch.cuda.get_device_name(0)}), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_samples.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.launches < 500:
        ap.error("at least 5 repeats of at least 500 launches")
    if args.child:
        child(args.child, args.repeats, args.launches)
        return 0
    lines = [f"ragged samples: skr_step_launch_rolling, {OPERANDS} bf16 operands and in-kernel noise, capacity {CAPACITY}, every slot active, through the C ABI; "
             f"{args.repeats} repeats of {args.launches} launches after {WARMUP} warm-up launches",
             EXPECTATION,
             "us per launch (HIP events): median (min - max) over the repeats; one child process per form"]  # fmt: skip
    print("\n".join(lines), flush=True)  # (the expectation is out before anything is measured)
    seen = {}
    for form in FORMS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--launches", str(args.launches), "--child", form],
                             capture_output=True, text=True, timeout=600)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return 1  # (nothing more is started on the device after a failure)
        seen[form] = json.loads(found[-1][len("RESULT "):])
    stats = {form: summary(seen[form]["event_us"]) for form in FORMS}
    measured = [f"({seen['r']['device']})"]
    for form, what in FORMS.items():
        m, lo, hi = stats[form]
        per_mb = f"   {m / algorithmic_mb(form):7.4f} us per algorithmic MB ({algorithmic_mb(form):.2f} MB)" if form != "e" else "   (64 calls)"
        measured.append(f"  {form}  {what:34s} {m:9.2f} ({lo:9.2f} - {hi:9.2f}){per_mb}")
    per = {form: [v / algorithmic_mb(form) for v in stats[form]] for form in ("r", "w")}
    excess = per["r"][0] / per["w"][0] - 1.0
    allowed = 32 / 31.5 - 1.0 + ((per["r"][2] - per["r"][1]) + (per["w"][2] - per["w"][1])) / per["w"][0]
    measured.append(f"  r against w per algorithmic byte: {100 * excess:+.2f} %; allowed {100 * (32 / 31.5 - 1):.2f} % + the two spreads together = {100 * allowed:.2f} %: "
                    f"the expectation {'held' if excess <= allowed else 'did NOT hold'}")  # fmt: skip
    measured.append(f"  e against r: {stats['e'][0] / stats['r'][0]:.2f} x the time of the one ragged launch")
    print("\n".join(measured))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + measured) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
