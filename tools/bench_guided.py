"""Cost of a guided step: SkrampleWrapperScheduler.step_guided against the three torch lines plus step() it replaces.
256 x (4, 128, 128) bf16 latents, Euler and DPM-2 (eta = 0), no network (a ring of fixed doubled-batch outputs, split with chunk(2)).

  python tools/bench_guided.py [--repeats 5] [--steps 200] [--out profiles/guided.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  guided step       latents = w.step_guided(uncond, cond, g, t, latents)
  b  torch lines       noise_pred = uncond + g * (cond - uncond);  latents = w.step(noise_pred, t, latents)
                       -- as users run it today: from the second run on the plain steps are served by the replayed fast path
  k  kernels alone     through the C ABI, at 3 and 4 operands: skr_step_launch_guided (storing p) back to back; beside it its
                       same-traffic twin, skr_step_launch in its two-output form with one operand more (as many reads and writes, the
                       parent's kernel); beside it the three torch kernels plus skr_step_launch.  Event clock per launch and the
                       fraction of 8 TB/s the algorithmic bytes come to (guided and twin: operands + cond + two stores; the torch
                       lines: 16 bytes per element, plus the step's operands and one store)
Per repeat, `steps` steps of a `steps`-step schedule are timed with HIP events (first enqueue to last kernel) and with the wall clock
(first call to the end of a device synchronisation); reported per form: median and min - max over the repeats, us per step.
Pass conditions: a's wall-clock median is below b's by more than the two forms' min - max spreads put together, for both samplers; the
guided kernel's median is below the median of "three torch kernels + step kernel" by more than their spreads put together.
Reported beside them, not judged: where the guided kernel stands against its same-traffic twin."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, WARMUP, SCALE = 256, (4, 128, 128), 20, 7.3
SAMPLERS = ("euler", "dpm2")
FORMS = {"a": "step_guided()", "b": "three torch lines + step()"}
PEAK = 8.0e12  # bytes per second


def child(form: str, sampler: str, repeats: int, steps: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    shape = (BATCH, *SHAPE)
    g = torch.Generator().manual_seed(1)
    fresh = lambda: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    result = {"form": form, "sampler": sampler, "device": torch.cuda.get_device_name(0)}

    def timed(launch):
        for _ in range(WARMUP):
            launch()
        torch.cuda.synchronize()
        per = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / steps)
        return per

    if form == "k":
        numel = BATCH * SHAPE[0] * SHAPE[1] * SHAPE[2]
        for n in (3, 4):
            ops, cond = [fresh() for _ in range(n)], fresh()
            out, guided = torch.empty_like(cond), torch.empty_like(cond)

            def plan_of(terms, two_outputs):
                plan = _hip.StepPlanC()
                plan.n_terms = plan.n_group_a = terms
                plan.dtype_a = plan.out0_dtype = _hip.BF16
                plan.dtype_b, plan.out1_dtype = _hip.F32, (_hip.BF16 if two_outputs else _hip.NONE)
                for k in range(terms):
                    plan.coef0[k], plan.coef1[k] = 0.5 - 0.1 * k, (0.25 if two_outputs else 0.0)
                return plan

            plain, twin = plan_of(n, False), plan_of(n + 1, True)

            def torch_lines_and_step():
                pred = ops[1] + SCALE * (cond - ops[1])
                _hip.launch_step(plain, [ops[0], pred, *ops[2:]], out, None, None, numel, dev)

            result[f"guided{n}_us"] = timed(lambda: _hip.launch_step_guided(plain, ops, out, cond, guided, SCALE, 1, None, numel, dev))
            result[f"twin{n}_us"] = timed(lambda: _hip.launch_step(twin, [*ops, cond], out, guided, None, numel, dev))
            result[f"lines{n}_us"] = timed(torch_lines_and_step)
            result[f"guided{n}_bytes"] = result[f"twin{n}_bytes"] = numel * 2 * (n + 1 + 2)
            result[f"lines{n}_bytes"] = numel * (16 + 2 * (n + 1))
        print("RESULT " + json.dumps(result), flush=True)
        return

    make = (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))) if sampler == "dpm2" else (lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled())))  # fmt: skip
    w = make()
    x0 = fresh()
    big = lambda: (torch.randn((2 * BATCH, *SHAPE), generator=g) * 0.1).bfloat16().to(dev)  # noqa: E731
    ring = [big().chunk(2) for _ in range(4)]  # (doubled-batch outputs: fresh memory to the history's alias guard, as a network's would be)

    def run(ts):
        x = x0
        if form == "a":
            for i, t in enumerate(ts):
                uncond, cond = ring[i & 3]
                x = w.step_guided(uncond, cond, SCALE, t, x, return_dict=False)[0]
        else:
            for i, t in enumerate(ts):
                uncond, cond = ring[i & 3]
                x = w.step(uncond + SCALE * (cond - uncond), t, x, return_dict=False)[0]
        return x

    def schedule():
        w.set_timesteps(steps)
        return w.timesteps.tolist()

    for _ in range(2):  # (two whole runs: the plain steps of form b are served by the replayed fast path from the second run on)
        run(schedule())
    torch.cuda.synchronize()
    event_us, wall_us = [], []
    for _ in range(repeats):
        ts = schedule()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        run(ts)
        e1.record()
        torch.cuda.synchronize()
        wall_us.append((time.perf_counter() - t0) * 1e6 / steps)
        event_us.append(e0.elapsed_time(e1) * 1e3 / steps)
    result.update(event_us=event_us, wall_us=wall_us, fast_hits=w._fast_hits)
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200:
        ap.error("at least 5 repeats of at least 200 steps")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.steps)
        return 0

    def spawn(form, sampler):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--child", form, sampler],
                             capture_output=True, text=True, timeout=600)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} / {sampler} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        return json.loads(found[-1][len("RESULT "):])

    lines = [f"guided steps: {BATCH} x {SHAPE} bf16 latents, guidance scale {SCALE}, no network; {args.repeats} repeats of {args.steps} steps after two warm-up runs",
             "us per step: median (min - max) over the repeats; one child process per form and sampler"]  # fmt: skip
    failed = False
    for sampler in SAMPLERS:
        seen = {}
        for form in FORMS:
            seen[form] = spawn(form, sampler)
            if seen[form] is None:
                return 1
        lines.append(f"{sampler}  ({seen['a']['device']})")
        for form, what in FORMS.items():
            (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
            lines.append(f"  {form}  {what:26s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})   fast-path steps {seen[form]['fast_hits']}")
        (am, alo, ahi), (bm, blo, bhi) = summary(seen["a"]["wall_us"]), summary(seen["b"]["wall_us"])
        margin = (ahi - alo) + (bhi - blo)
        ok = bm - am > margin
        failed |= not ok
        lines.append(f"  wall-clock medians: b - a = {bm - am:.2f} us (b / a = {bm / am:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (a below b by more than the spreads)")
        (eam, _, _), (ebm, _, _) = summary(seen["a"]["event_us"]), summary(seen["b"]["event_us"])
        lines.append(f"  event-clock medians: b / a = {ebm / eam:.2f}")
    k = spawn("k", "none")
    if k is None:
        return 1
    lines.append("kernels alone, through the C ABI")
    for n in (3, 4):
        for name, what in (("guided", "skr_step_launch_guided"), ("twin", "two-output skr_step_launch"), ("lines", "3 torch kernels + step")):
            m, lo, hi = summary(k[f"{name}{n}_us"])
            lines.append(f"  k  {what:28s} {n} operands   event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f}) per launch   {k[f'{name}{n}_bytes'] / 1e6:7.1f} MB -> {k[f'{name}{n}_bytes'] / (m * 1e-6) / PEAK * 100:5.1f} % of 8 TB/s")
        (gm, glo, ghi), (lm, llo, lhi), (tm, tlo, thi) = summary(k[f"guided{n}_us"]), summary(k[f"lines{n}_us"]), summary(k[f"twin{n}_us"])
        margin = (ghi - glo) + (lhi - llo)
        ok = lm - gm > margin
        failed |= not ok
        lines.append(f"  k  {n} operands: lines - guided = {lm - gm:.2f} us (lines / guided = {lm / gm:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'}")
        lines.append(f"  k  {n} operands: guided median {gm:.2f} us against its same-traffic twin's {tm:.2f} ({tlo:.2f} - {thi:.2f}): {'inside' if tlo <= gm <= thi else 'outside'} the twin's spread (not judged)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
