"""Cost of the row forms of the guided step: the kernels against their kernarg twin, and a captured guided loop against what a user
could capture before it.  256 x (4, 128, 128) bf16 latents.

  python tools/bench_guided_rows.py [--repeats 5] [--steps 200] [--out profiles/guided_rows.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  k  kernels alone     through the C ABI, at 3 and 4 operands, storing p: skr_step_launch_guided (the yardstick, untouched),
                       skr_step_launch_guided_indexed and skr_step_launch_guided_indexed_per_sample, each back to back; the three take
                       turns within every repeat.  Event clock per launch.
  g  guided loop       capture_sampling_loop(DPM-2, indexed=True, guidance_scale=7.5) over an elementwise two-output network: per step
                       the network's two kernels and ONE guided row launch
  y  yardstick loop    what a user can capture without the row forms: the same indexed loop whose model returns u + g * (c - u) -- the
                       network's two kernels, torch's three, then the plain indexed step launch
Loops are LOOP_STEPS long and replayed steps / LOOP_STEPS times per repeat, timed with HIP events around the replays (graph.replay()
alone: no copy in, no clone out); reported per form: median and min - max over the repeats, us per step.
Expectations, stated before the run: (a) the row kernels equal the kernarg twin within the two spreads together, or sit above it by one
dependent scalar load (DESIGN.md section 8 measured 0.77 us for the rolling noise kernels); reported, not judged.  (b) the kernel-level
2x of DESIGN.md section 4.7 appears as a difference of about one step-kernel time per step (~30 us).
Pass condition (b): g's median is below y's by more than the two forms' min - max spreads put together."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, WARMUP, SCALE, LOOP_STEPS = 256, (4, 128, 128), 20, 7.5, 50
LOOPS = {"g": "guided loop (row launch)", "y": "torch lines in the model + step"}
KERNELS = (("kernarg", "skr_step_launch_guided"), ("indexed", "skr_step_launch_guided_indexed"), ("per_sample", "skr_step_launch_guided_indexed_per_sample"))


def child(form: str, repeats: int, steps: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.graphs import capture_sampling_loop
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    shape = (BATCH, *SHAPE)
    g = torch.Generator().manual_seed(1)
    fresh = lambda: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    result = {"form": form, "device": torch.cuda.get_device_name(0)}

    def timed_once(launch, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(count):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    if form == "k":
        lib = _hip.load()
        numel = BATCH * SHAPE[0] * SHAPE[1] * SHAPE[2]
        stream = _hip.current_stream_ptr(dev)
        for n in (3, 4):
            ops, cond = [fresh() for _ in range(n)], fresh()
            out, guided = torch.empty_like(cond), torch.empty_like(cond)
            plan = _hip.StepPlanC()
            plan.n_terms = plan.n_group_a = n
            plan.dtype_a = plan.out0_dtype = _hip.BF16
            plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
            plan.sample_numel = numel // BATCH
            row = _hip.StepRowC()
            for k in range(n):
                plan.coef0[k] = row.coef0[k] = 0.5 - 0.1 * k
            row.convert_k[0] = SCALE
            table = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
            _hip.upload_rows(table, 0, [row])
            index, sample_index = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(BATCH, dtype=torch.int32, device=dev)
            arr = _hip._operand_array(ops)
            guide = _hip.StepGuidanceC(cond.data_ptr(), guided.data_ptr(), SCALE, 1, 0)
            head = (ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), None, numel)

            def run(status):
                if status != 0:
                    raise SystemExit(f"launch refused with status {status}")

            launches = {
                "kernarg": lambda: run(lib.skr_step_launch_guided(*head, stream)),
                "indexed": lambda: run(lib.skr_step_launch_guided_indexed(*head, table.data_ptr(), index.data_ptr(), 0, stream)),
                "per_sample": lambda: run(lib.skr_step_launch_guided_indexed_per_sample(*head, table.data_ptr(), sample_index.data_ptr(), 0, stream)),
            }
            wants = {}
            for name, launch in launches.items():  # (the three forms write the same bits: checked at the size that is timed)
                out.zero_(), guided.zero_()
                launch()
                wants[name] = (out.clone(), guided.clone())
            result[f"same_bits{n}"] = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for name in ("indexed", "per_sample") for a, b in zip(wants[name], wants["kernarg"]))
            for launch in launches.values():
                timed_once(launch, WARMUP)
            per = {name: [] for name in launches}
            for _ in range(repeats):
                for name, launch in launches.items():  # the forms take turns within a repeat
                    per[name].append(timed_once(launch, steps) / steps)
            for name in launches:
                result[f"{name}{n}_us"] = per[name]
        print("RESULT " + json.dumps(result), flush=True)
        return

    def net(x, t):  # elementwise, two outputs: the halves of a doubled-batch network output
        return x * 0.5, x * 0.25

    def lines(x, t):  # what a user writes inside the captured model without the guided row launch
        u, c = net(x, t)
        return u + SCALE * (c - u)

    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    x0 = fresh()
    if form == "g":
        loop = capture_sampling_loop(w, net, x0, LOOP_STEPS, indexed=True, guidance_scale=SCALE)
    else:
        loop = capture_sampling_loop(w, lines, x0, LOOP_STEPS, indexed=True)
    result["launches_per_loop"] = loop.rows.length
    result["checksum"] = float(loop(x0).float().abs().mean())  # (the two forms compute the same loop: printed beside the times)
    replays = steps // LOOP_STEPS
    timed_once(loop.graph.replay, 2)
    result["event_us"] = [timed_once(loop.graph.replay, replays) / (replays * LOOP_STEPS) for _ in range(repeats)]
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_rows.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200 or args.steps % LOOP_STEPS != 0:
        ap.error(f"at least 5 repeats of at least 200 steps, a multiple of {LOOP_STEPS}")
    if args.child:
        child(args.child, args.repeats, args.steps)
        return 0

    def spawn(form):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--child", form],
                             capture_output=True, text=True, timeout=600)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        return json.loads(found[-1][len("RESULT "):])

    k = spawn("k")
    if k is None:
        return 1
    lines = [f"guided steps with device-resident rows: {BATCH} x {SHAPE} bf16 latents, guidance scale {SCALE}; {args.repeats} repeats of {args.steps} steps  ({k['device']})",
             "us: median (min - max) over the repeats; one child process per form",
             "(a) kernels alone, through the C ABI, storing p; the three forms take turns within every repeat"]  # fmt: skip
    for n in (3, 4):
        (km, klo, khi) = summary(k[f"kernarg{n}_us"])
        for name, what in KERNELS:
            m, lo, hi = summary(k[f"{name}{n}_us"])
            lines.append(f"  k  {what:42s} {n} operands   event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f}) per launch")
        for name in ("indexed", "per_sample"):
            m, lo, hi = summary(k[f"{name}{n}_us"])
            margin = (hi - lo) + (khi - klo)
            verdict = "equal within the two spreads together" if abs(m - km) <= margin else ("above the kernarg twin" if m > km else "below the kernarg twin")
            lines.append(f"  k  {n} operands: {name} - kernarg = {m - km:+.2f} us, the two spreads together {margin:.2f} us: {verdict} (reported, not judged)")
        lines.append(f"  k  {n} operands: the three forms wrote the same bits at this size: {k[f'same_bits{n}']}")
    seen = {}
    for form in LOOPS:
        seen[form] = spawn(form)
        if seen[form] is None:
            return 1
    lines.append(f"(b) captured indexed DPM-2 loops of {LOOP_STEPS} steps over an elementwise two-output network, replayed {args.steps // LOOP_STEPS} times per repeat; us per step")
    for form, what in LOOPS.items():
        m, lo, hi = summary(seen[form]["event_us"])
        lines.append(f"  {form}  {what:34s} event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f})   step launches per loop {seen[form]['launches_per_loop']}   mean |x| {seen[form]['checksum']:.6f}")
    (gm, glo, ghi), (ym, ylo, yhi) = summary(seen["g"]["event_us"]), summary(seen["y"]["event_us"])
    margin = (ghi - glo) + (yhi - ylo)
    ok = ym - gm > margin
    lines.append(f"  medians: y - g = {ym - gm:.2f} us per step (y / g = {ym / gm:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (g below y by more than the spreads)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
