"""Cost of one projected-guidance tick of a rolling batch against the per-sample row pair and against torch's lines, through the C ABI:
capacity 64 x (4, 128, 128) bf16, DPM-2 rows (three operands: sample, uncond, the previous prediction; no draw), every row a momentum row
(g 7.5, eta 0, a norm threshold that clamps, beta -0.5).

  python tools/bench_projected_rolling.py [--repeats 5] [--ticks 2000] [--out profiles/projected_guidance_rolling.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  per-sample pair            skr_projected_guidance_coef_indexed_per_sample + skr_projected_guided_step_launch_indexed_per_sample: the
                                yardstick, code this change does not touch
  b  rolling, 64 of 64 active   skr_projected_guidance_coef_rolling + skr_projected_guided_step_launch_rolling, every slot at a position of
                                its own
  c  rolling, 16 of 64 active   the same, every fourth slot active: the other 48 slots' workgroups leave on their first scalar branch
  e  rolling, 0 of 64 active    the same with no slot active: what three launches a tick cost when every workgroup leaves at once -- the floor
                                under c: launch and dispatch cost, no memory traffic
  d  torch's lines + plain step the pipeline's APG lines (tools/bench_projected_guidance.py, apg_lines) over the whole batch, one setting
                                for all, then skr_step_launch_rolling: the route a server has without this change
A tick is the statistic, then the step, on one index vector; the index moves on with every tick, as a rolling batch's does.  Per repeat,
`ticks` ticks are timed with HIP events (first enqueue to last kernel) after a warm-up of 30.  The forms run in turn, twice over (a b c e d
a b c e d), so that a drift of the machine shows inside every form's spread; reported per form: median and min - max over the repeats of
both passes, us per tick.  The expectation is written into the profile ahead of the numbers; nothing is tuned to meet it."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CAPACITY, SHAPE, WARMUP, STEPS = 64, (4, 128, 128), 30, 32
G, ETA, BETA = 7.5, 0.0, -0.5
FORMS = {"a": "per-sample pair", "b": "rolling, 64 of 64 active", "c": "rolling, 16 of 64 active", "e": "rolling, 0 of 64 active", "d": "torch's lines + plain step"}
EXPECTATION = [
    "expectation, written before the run: the pair moves ten images of 8 MiB a tick (u, c, m in and d out in the statistic; x, d, c, h in and out, p out",
    "in the step), HBM-bound, so a (the per-sample pair) is expected where profiles/projected_guidance_rows.txt has it; b within the run-to-run spread of a",
    "-- the same traffic on the same grid, the index round trip in front of the loads hidden by the other workgroups of a 4096-workgroup launch --; c near",
    "a quarter of b unless three launches a tick cannot be enqueued that fast, which e (no slot active) shows; d at twice a or more (profiles/projected_guidance.txt:",
    "there one setting and no step; here the lines run eagerly on 64 samples).",
]


def child(form: str, repeats: int, ticks: int) -> None:
    import torch

    from skrample_amd import _hip

    dev = torch.device("cuda:0")
    lib, stream = _hip.load(), _hip.current_stream_ptr(dev)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    g = torch.Generator().manual_seed(1)
    x, u, c, h = (torch.randn(CAPACITY, n, generator=g).bfloat16().to(dev) for _ in range(4))
    mom, out, p = torch.zeros_like(x), torch.empty_like(x), torch.empty_like(x)
    r = 0.5 * float((c.double() - u.double()).norm(dim=1).mean())  # a threshold that clamps
    rows = []
    for k in range(CAPACITY * STEPS):  # every slot's own run of DPM-2-like rows; a run's first row starts its running average
        row = _hip.StepRowC()
        row.coef0[0], row.coef0[1], row.coef0[2] = 0.7 + 1e-3 * (k % STEPS), 0.9, -0.4
        row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3] = G, ETA, r, BETA
        row.stream1 = 1 if k % STEPS == 0 and form != "a" else 0
        rows.append(row)
    table = torch.zeros(len(rows) * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
    _hip.upload_rows(table, 0, rows)
    total = WARMUP + repeats * ticks
    slots = torch.arange(CAPACITY, dtype=torch.int64)
    live = (slots % 4 == 0) if form == "c" else torch.zeros(CAPACITY, dtype=torch.bool) if form == "e" else torch.ones(CAPACITY, dtype=torch.bool)
    index = torch.where(live[None, :], slots[None, :] * STEPS + (torch.arange(total, dtype=torch.int64)[:, None] + slots[None, :]) % STEPS, torch.full((1, 1), -1, dtype=torch.int64))
    index = index.to(torch.int32).to(dev)
    first, stride = index.data_ptr(), CAPACITY * index.element_size()  # (tick t reads row t: no tensor indexing inside the timed loop)
    coef = torch.zeros(2 * CAPACITY, dtype=torch.float32, device=dev)
    partials = torch.zeros(_hip.projected_partials(CAPACITY * n, n), dtype=torch.float64, device=dev)
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 3
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype, plan.sample_numel = _hip.NONE, n  # (the plain rolling step of form d finds its slots by it)
    guide, proj = _hip.StepGuidanceC(c.data_ptr(), p.data_ptr(), 0.0, 1, 0), _hip.StepProjectionC(coef.data_ptr(), mom.data_ptr(), n, 0)
    arr = _hip._operand_array([x, u, h])

    if form == "d":
        from bench_projected_guidance import apg_lines

        shaped, state = (CAPACITY, *SHAPE), {"m": mom.view(CAPACITY, *SHAPE)}

        def tick(t):
            guided = apg_lines(u.view(shaped), c.view(shaped), G, ETA, r, BETA, state).contiguous()
            values = dict(plan=plan, operands=_hip._operand_array([x, guided.view(CAPACITY, n), h]), out0=out.data_ptr(), out1=None, seeds=None, numel=CAPACITY * n,
                          rows=table.data_ptr(), index=first + t * stride, row_offset=0, stream=stream)  # fmt: skip
            return _hip.call_entry(lib, "plain", "rolling", values)
    else:
        suffix = "_indexed_per_sample" if form == "a" else "_rolling"
        statistic, step = getattr(lib, "skr_projected_guidance_coef" + suffix), getattr(lib, "skr_projected_guided_step_launch" + suffix)

        def tick(t):
            at = first + t * stride
            return (statistic(u.data_ptr(), c.data_ptr(), mom.data_ptr(), _hip.BF16, CAPACITY * n, n, table.data_ptr(), at, 0, coef.data_ptr(), None, partials.data_ptr(), stream)
                    | step(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(proj), None, CAPACITY * n, table.data_ptr(), at, 0, stream))  # fmt: skip

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
    assert form == "e" or torch.isfinite(out[live.to(dev)].float()).all()
    print("RESULT " + json.dumps({"form": form, "event_us": event_us, "device": f"{torch.cuda.get_device_name(0)}, {getattr(torch.cuda.get_device_properties(0), 'gcnArchName', 'architecture not reported')}"}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projected_guidance_rolling.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.ticks < 100:
        ap.error("at least 5 repeats of at least 100 ticks")
    if args.child:
        child(args.child, args.repeats, args.ticks)
        return 0
    lines = [f"projected-guidance ticks: capacity {CAPACITY} x {SHAPE} bf16, DPM-2 rows, through the C ABI; two passes of {args.repeats} repeats of {args.ticks} ticks after {WARMUP} warm-up ticks",
             *EXPECTATION, "us per tick (HIP events): median (min - max) over the repeats; one child process per form"]  # fmt: skip
    seen = {}
    for form in [*FORMS, *FORMS]:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--ticks", str(args.ticks), "--child", form],
                             capture_output=True, text=True, timeout=300)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return 1  # (nothing more is started on the device after a failure)
        result = json.loads(found[-1][len("RESULT "):])
        seen.setdefault(form, result)["event_us"] = seen.get(form, {"event_us": []})["event_us"] + result["event_us"]
    stats = {form: (statistics.median(v), min(v), max(v)) for form, v in ((f, seen[f]["event_us"]) for f in FORMS)}
    lines.append(f"({seen['a']['device']})")
    for form, what in FORMS.items():
        m, lo, hi = stats[form]
        lines.append(f"  {form}  {what:26s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
    spread = lambda form: stats[form][2] - stats[form][1]  # noqa: E731
    ab, bc = stats["b"][0] - stats["a"][0], stats["b"][0] - stats["c"][0]
    lines.append(f"  b - a = {ab:+.2f} us ({100 * ab / stats['a'][0]:+.1f} %); the two spreads together {spread('a') + spread('b'):.2f} us: the row in front of the loads costs "
                 f"{'no more than' if ab <= spread('a') + spread('b') else 'MORE than'} the run-to-run spread")  # fmt: skip
    lines.append(f"  b - c = {bc:+.2f} us (c is {stats['c'][0] / stats['b'][0]:.2f} of b with a quarter of the slots active); the two spreads together {spread('b') + spread('c'):.2f} us: "
                 f"inactive slots are {'cheaper' if bc > spread('b') + spread('c') else 'NOT cheaper'}")  # fmt: skip
    lines.append(f"  c - e = {stats['c'][0] - stats['e'][0]:+.2f} us: what 16 active slots add to three launches that touch no memory")
    lines.append(f"  d / b = {stats['d'][0] / stats['b'][0]:.2f}: torch's lines over the whole batch plus the plain rolling step against the two rolling launches")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
