"""Cost of adaptive projected guidance in a captured loop: a DPM-2 loop of bf16 latents, no network (a ring of fixed halves), at
64 x (4, 128, 128) and 64 x (3, 64, 64), three routes:

  rows   capture_sampling_loop(..., indexed=True, guidance_scale=g, projected=True): every step the statistics row launch and the row step
  torch  what could be captured without the row forms: an indexed loop whose model returns torch's APG lines (running average, norm
         clamp, projection on float64 tensors, guided sum) as the prediction, stepped by the plain row launch
  eager  the eager step_guided() loop under set_projected_guidance

  python tools/bench_projected_rows.py [--rounds 3] [--repeats 5] [--steps 48] [--out profiles/projected_guidance_rows.txt]

The routes alternate, each run in a child process of its own (a fresh HIP context and allocator; the parent never opens the GPU): `rounds`
times rows, torch, eager, ...  Per child `repeats` runs of `steps` steps (a replay of the captured loop, or the eager loop) are timed with
HIP events after two warm-up runs; reported per route and size: median and min - max over every repeat of every round, us per step.  rows
is called faster than another route only where that route's median exceeds its own by more than the two min - max spreads together;
otherwise the line says so.
A fourth child times the step launches alone through the C ABI, 3 operands, slot 1: skr_projected_guided_step_launch with and without
diff (the compile-time split of projected_kernel_v1) against skr_projected_guided_step_launch_indexed on a momentum row and on a
zero-momentum row (the run-time choice), alternating, us per launch over back-to-back launches on the event clock."""

import argparse
import ctypes
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_projected_guidance import BETA, ETA, SCALE, SIZES, apg_lines, summary  # noqa: E402

ROUTES = {"rows": "captured, projected=True (row launches)", "torch": "captured, torch APG lines + plain row step", "eager": "eager step_guided"}


def timed(fn, repeats, per):
    "us per `per` units of work over `repeats` timed calls of fn, after two warm-up calls"
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    found = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        found.append(e0.elapsed_time(e1) * 1e3 / per)
    return found


def child(form: str, size: str, repeats: int, steps: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip, graphs
    from skrample_amd.sampling import structured as PT

    dev, shape = torch.device("cuda:0"), SIZES[size]
    g = torch.Generator().manual_seed(1)
    fresh = lambda: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    ring = [(fresh(), fresh()) for _ in range(4)]
    x0 = fresh()
    r = 0.5 * float((ring[0][1].double() - ring[0][0].double()).reshape(shape[0], -1).norm(dim=1).mean())  # a threshold that clamps
    result = {"form": form, "size": size, "device": torch.cuda.get_device_name(0)}

    if form == "kernels":
        lib, numel, n = _hip.load(), x0.numel(), x0.numel() // shape[0]
        (u, c), m, prev, out, p = ring[0], ring[1][0], ring[1][1], torch.empty_like(x0), torch.empty_like(x0)
        coef = torch.ones(2 * shape[0], dtype=torch.float32, device=dev)
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = 3
        plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
        plan.out1_dtype = _hip.NONE
        plan.coef0[0], plan.coef0[1], plan.coef0[2] = 0.9, 0.3, -0.2
        table = []
        for beta in (BETA, 0.0):
            row = _hip.IndexedRows.row_from(plan)
            row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3] = SCALE, ETA, r, beta
            table.append(row)
        rows_dev = torch.zeros(2 * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
        _hip.upload_rows(rows_dev, 0, table)
        arr, guide = (ctypes.c_void_p * 3)(x0.data_ptr(), u.data_ptr(), prev.data_ptr()), _hip.StepGuidanceC(c.data_ptr(), p.data_ptr(), 0.0, 1, 0)
        with_diff, without = _hip.StepProjectionC(coef.data_ptr(), m.data_ptr(), n, 0), _hip.StepProjectionC(coef.data_ptr(), None, n, 0)
        stream = _hip.current_stream_ptr(dev)

        def direct(proj):
            return lambda: [_hip.check(lib.skr_projected_guided_step_launch(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(proj), None, numel, stream),
                                       "skr_projected_guided_step_launch") for _ in range(steps)]  # fmt: skip

        def row(k):
            return lambda: [_hip.check(lib.skr_projected_guided_step_launch_indexed(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(with_diff), None,
                                                                                     numel, rows_dev.data_ptr(), None, k, stream),
                                       "skr_projected_guided_step_launch_indexed") for _ in range(steps)]  # fmt: skip

        routes = {"direct_diff": direct(with_diff), "row_momentum": row(0), "direct_uncond": direct(without), "row_zero_momentum": row(1)}
        found = {name: [] for name in routes}
        for _ in range(3):  # alternating
            for name, fn in routes.items():
                found[name] += timed(fn, repeats, steps)
        result.update(kernels=found)
        print("RESULT " + json.dumps(result), flush=True)
        return

    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    if form != "torch":
        w.set_projected_guidance(eta=ETA, norm_threshold=r, momentum=BETA)
    calls = itertools.count()
    pair = lambda x, t: ring[next(calls) & 3]  # noqa: E731  (steps is a multiple of 4: every run of the loop sees the same halves)
    if form == "rows":
        loop = graphs.capture_sampling_loop(w, pair, x0, steps, indexed=True, guidance_scale=SCALE, projected=True)
        run = lambda: loop.graph.replay()  # noqa: E731
    elif form == "torch":
        state = {}

        def model(x, t):
            i = next(calls)
            if i % steps == 0:
                state["m"] = torch.zeros_like(x0)  # a new run: the running average starts from zero
            return apg_lines(*ring[i & 3], SCALE, ETA, r, BETA, state)

        loop = graphs.capture_sampling_loop(w, model, x0, steps, indexed=True)
        run = lambda: loop.graph.replay()  # noqa: E731
    else:

        def run():
            w.set_timesteps(steps)
            x = x0
            for t in w.timesteps.tolist():
                x = w.step_guided(*pair(x, t), SCALE, t, x, return_dict=False)[0]

    result.update(event_us=timed(run, repeats, steps))
    print("RESULT " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projected_guidance_rows.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SIZE"))
    args = ap.parse_args()
    if args.steps % 4 != 0:
        ap.error("--steps must be a multiple of 4 (the ring of halves)")
    if args.child:
        child(*args.child, args.repeats, args.steps)
        return 0

    def spawn(form, size):
        print(f"[{form} at {size}]", file=sys.stderr, flush=True)
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--child", form, size],
                             capture_output=True, text=True, timeout=300)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} at {size} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        return json.loads(found[-1][len("RESULT "):])

    lines = [f"adaptive projected guidance in a captured DPM-2 loop: bf16, guidance scale {SCALE}, eta {ETA}, momentum {BETA}, a threshold that clamps, no network; "
             f"{args.rounds} alternating rounds of {args.repeats} repeats of {args.steps} steps, one child process per route and round",
             "us per step on the event clock: median (min - max) over all repeats"]  # fmt: skip
    for size in SIZES:
        seen = {form: [] for form in ROUTES}
        for _ in range(args.rounds):
            for form in ROUTES:
                got = spawn(form, size)
                if got is None:
                    return 1
                seen[form] += got["event_us"]
        lines.append(f"64 x {size}  ({got['device']})")
        stats = {form: summary(values) for form, values in seen.items()}
        for form, what in ROUTES.items():
            m, lo, hi = stats[form]
            lines.append(f"  {form:6s} {what:44s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
        am, alo, ahi = stats["rows"]
        for other in ("torch", "eager"):
            om, olo, ohi = stats[other]
            margin = (ahi - alo) + (ohi - olo)
            verdict = f"rows is faster: rows / {other} = {am / om:.2f}" if om - am > margin else "NO speed-up claimed: the difference does not exceed the spreads"
            lines.append(f"  {other} - rows = {om - am:.2f} us, the two spreads together {margin:.2f} us: {verdict}")
        got = spawn("kernels", size)
        if got is None:
            return 1
        lines.append(f"  step launch alone, 3 operands, us per launch over {args.steps} back-to-back launches:")
        for name, values in got["kernels"].items():
            m, lo, hi = summary(values)
            lines.append(f"    {name:18s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
