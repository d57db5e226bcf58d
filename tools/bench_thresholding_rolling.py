"""Cost of one thresholded tick of a rolling batch against the per-sample row pair, through the C ABI: capacity 64 x (4, 128, 128) bf16,
DPM-2 rows (three operands: sample, network output, the previous prediction; no draw), every row selecting (ratio 0.995, maximum 1e30).

  python tools/bench_thresholding_rolling.py [--repeats 7] [--ticks 300] [--out profiles/thresholding_rolling.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  per-sample pair            skr_threshold_scale_indexed_per_sample + skr_thresholded_step_launch_indexed_per_sample: the yardstick,
                                code this change does not touch
  b  rolling, 64 of 64 active   skr_threshold_scale_rolling + skr_thresholded_step_launch_rolling, every slot at a position of its own
  c  rolling, 16 of 64 active   the same, every fourth slot active: the other 48 slots' workgroups leave on their first scalar branch
A tick is the statistic, then the step, on one index vector; the index moves on with every tick, as a rolling batch's does.  Per repeat,
`ticks` ticks are timed with HIP events (first enqueue to last kernel) after a warm-up of 30; reported per form: median and min - max over
the repeats, us per tick.  The expectation is written into the profile ahead of the numbers, and the pass condition is stated with them:
b is not above a by more than the two spreads together plus the index round trip of the five kernels that have it (0.77 us each in
profiles/rolling_noise.txt), and c is below b by more than the spreads."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, SHAPE, WARMUP, STEPS = 64, (4, 128, 128), 30, 32
ROUND_TRIP_US, KERNELS = 0.77, 5
FORMS = {"a": "per-sample pair", "b": "rolling, 64 of 64 active", "c": "rolling, 16 of 64 active"}
EXPECTATION = [
    "expectation, written before the run: the statistic is 100 - 104 us of ballot loops and atomics in every row form (profiles/thresholding_rows.txt)",
    "and the step about 3 us, so a (the per-sample pair) is expected near 105 us; b within a few us of a -- the same passes on the same grid, plus one",
    f"index round trip in front of {KERNELS} kernels ({KERNELS} x {ROUND_TRIP_US} us) --; c near a quarter of b, since 48 of 64 slots end before they touch memory and",
    "the statistic's time is per-sample work, though the finish pass (one workgroup a slot) and launch gaps do not shrink with it.",
]


def child(form: str, repeats: int, ticks: int) -> None:
    import torch

    from skrample_amd import _hip

    dev = torch.device("cuda:0")
    lib, stream = _hip.load(), _hip.current_stream_ptr(dev)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    g = torch.Generator().manual_seed(1)
    x, o, h = ((torch.randn(CAPACITY, n, generator=g) * 2).bfloat16().to(dev) for _ in range(3))
    out, p = torch.empty_like(x), torch.empty_like(x)
    rows = []
    for k in range(CAPACITY * STEPS):  # every slot's own run of DPM-2-like rows
        row = _hip.StepRowC()
        row.coef0[0], row.coef0[1], row.coef0[2] = 0.7 + 1e-3 * (k % STEPS), 0.9, -0.4
        row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3] = 1.25, -0.75, 0.995, 1e30
        rows.append(row)
    table = torch.zeros(len(rows) * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
    _hip.upload_rows(table, 0, rows)
    total = WARMUP + repeats * ticks
    slots = torch.arange(CAPACITY, dtype=torch.int64)
    live = (slots % 4 == 0) if form == "c" else torch.ones(CAPACITY, dtype=torch.bool)
    index = torch.where(live[None, :], slots[None, :] * STEPS + (torch.arange(total, dtype=torch.int64)[:, None] + slots[None, :]) % STEPS, torch.full((1, 1), -1, dtype=torch.int64))
    index = index.to(torch.int32).to(dev)
    first, stride = index.data_ptr(), CAPACITY * index.element_size()  # (tick t reads row t: no tensor indexing inside the timed loop)
    scale = torch.zeros(CAPACITY, dtype=torch.float32, device=dev)
    workspace = torch.zeros(_hip.threshold_workspace(CAPACITY * n, n), dtype=torch.uint8, device=dev)
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 3
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    thr = _hip.StepThresholdC(scale.data_ptr(), p.data_ptr(), 0.0, 0.0, n, 1, 0, 0)
    arr = _hip._operand_array([x, o, h])
    suffix = "_indexed_per_sample" if form == "a" else "_rolling"
    statistic, step = getattr(lib, "skr_threshold_scale" + suffix), getattr(lib, "skr_thresholded_step_launch" + suffix)

    def tick(t):
        at = first + t * stride
        return (statistic(x.data_ptr(), o.data_ptr(), _hip.BF16, CAPACITY * n, n, table.data_ptr(), at, 0, scale.data_ptr(), workspace.data_ptr(), stream)
                | step(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(thr), None, CAPACITY * n, table.data_ptr(), at, 0, stream))  # fmt: skip

    t = 0
    for _ in range(WARMUP):
        _hip.check(tick(t), "tick")
        t += 1
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = 0
        for _ in range(ticks):
            status |= tick(t)
            t += 1
        e1.record()
        torch.cuda.synchronize()
        _hip.check(status, "tick")
        event_us.append(e0.elapsed_time(e1) * 1e3 / ticks)
    assert torch.isfinite(out[live.to(dev)].float()).all() and (scale[live.to(dev)] >= 1.0).all()
    print("RESULT " + json.dumps({"form": form, "event_us": event_us, "device": f"{torch.cuda.get_device_name(0)}, {getattr(torch.cuda.get_device_properties(0), 'gcnArchName', 'architecture not reported')}"}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thresholding_rolling.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.ticks < 100:
        ap.error("at least 5 repeats of at least 100 ticks")
    if args.child:
        child(args.child, args.repeats, args.ticks)
        return 0
    lines = [f"thresholded ticks: capacity {CAPACITY} x {SHAPE} bf16, DPM-2 rows, through the C ABI; {args.repeats} repeats of {args.ticks} ticks after {WARMUP} warm-up ticks",
             *EXPECTATION, "us per tick (HIP events): median (min - max) over the repeats; one child process per form"]  # fmt: skip
    seen = {}
    for form in FORMS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--ticks", str(args.ticks), "--child", form],
                             capture_output=True, text=True, timeout=300)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return 1  # (nothing more is started on the device after a failure)
        seen[form] = json.loads(found[-1][len("RESULT "):])
    stats = {form: (statistics.median(v), min(v), max(v)) for form, v in ((f, seen[f]["event_us"]) for f in FORMS)}
    lines.append(f"({seen['a']['device']})")
    for form, what in FORMS.items():
        m, lo, hi = stats[form]
        lines.append(f"  {form}  {what:26s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
    spread = lambda form: stats[form][2] - stats[form][1]  # noqa: E731
    ab, bc = stats["b"][0] - stats["a"][0], stats["b"][0] - stats["c"][0]
    allowed = spread("a") + spread("b") + KERNELS * ROUND_TRIP_US
    lines.append(f"  b - a = {ab:+.2f} us ({100 * ab / stats['a'][0]:+.1f} %); allowed: the two spreads together {spread('a') + spread('b'):.2f} us plus {KERNELS} x {ROUND_TRIP_US} us = "
                 f"{allowed:.2f} us: {'PASS' if ab <= allowed else 'FAIL'}")  # fmt: skip
    lines.append(f"  b - c = {bc:+.2f} us (c is {stats['c'][0] / stats['b'][0]:.2f} of b with a quarter of the slots active); the two spreads together {spread('b') + spread('c'):.2f} us: "
                 f"{'PASS' if bc > spread('b') + spread('c') else 'FAIL'}")  # fmt: skip
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
