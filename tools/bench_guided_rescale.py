"""Cost of rescaled guidance (guidance_rescale): the statistics launch plus the rescaled guided step against what a user runs today --
torch's nine kernels (three guidance lines, two whole-sample stds, the division aside, four elementwise lines) and then the step.
256 x (4, 128, 128) bf16 latents, DPM-2 (eta = 0), no network (a ring of fixed doubled-batch outputs, split with chunk(2)).

  python tools/bench_guided_rescale.py [--repeats 7] [--steps 200] [--out profiles/guided_rescale.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  k   kernels alone    through the C ABI, at 3 and 4 operands: skr_guidance_rescale_factor + skr_step_launch_guided_rescaled (storing p')
                       back to back, against torch's lines + skr_step_launch; and the statistics launch by itself, with the fraction of
                       8 TB/s its two tensor reads come to (what says whether it is HBM-bound)
  ln  captured loop    capture_sampling_loop(..., guidance_scale=g, guidance_rescale=phi), indexed=False, replayed
  lo  captured loop    the loop a user can capture today: the model returns the torch lines, then step(); replayed
  en  eager call       w.step_guided(uncond, cond, g, t, x, guidance_rescale=phi)             (reported, not judged: host-bound)
  eo  eager call       w.step(torch lines, t, x)                                              (reported, not judged)
  r   for the record   how many samples get the factor of torch's OWN device std, and how many elements of the rescaled prediction
                       differ where they do not (bf16 and fp32, 64 samples of (4, 32, 32) each)
Expectation from the byte counts, written before the run: with n step operands the new form moves 2 (statistic) + n + 1 + 2 tensor
passes, torch's lines 3 + 2 + 3 + 1 + 1 + 2 + 2 + 2 + 3 = 19 and the step n + 1: 8 against 23 at n = 3 (0.35), 9 against 24 at n = 4 (0.38).
Per repeat, `steps` steps are timed with HIP events (first enqueue to last kernel); eager forms also with the wall clock (first call to
the end of a device synchronisation); reported per form: median and min - max over the repeats, us per step.
Pass conditions (the project's rule): the new form's median is below the yardstick's by more than the two forms' min - max spreads put
together -- for the kernels alone at 3 and at 4 operands, and for the captured loop.  A condition that fails is written as FAIL."""

import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, WARMUP, SCALE, PHI = 256, (4, 128, 128), 20, 7.3, 0.7
FORMS = {"ln": "captured loop, guidance_rescale", "lo": "captured loop, torch lines + step()", "en": "eager step_guided(guidance_rescale)", "eo": "eager torch lines + step()"}
PEAK = 8.0e12  # bytes per second
EXPECTED = {3: (8, 23), 4: (9, 24)}  # tensor passes: new form, yardstick


def torch_lines(u, c, scale, phi):
    "what the pipeline runs today: the three guidance lines and rescale_noise_cfg"
    p = u + scale * (c - u)
    std_text = c.std(dim=list(range(1, c.ndim)), keepdim=True)
    std_cfg = p.std(dim=list(range(1, p.ndim)), keepdim=True)
    resc = p * (std_text / std_cfg)
    return phi * resc + (1 - phi) * p


def child(form: str, repeats: int, steps: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.graphs import capture_sampling_loop
    from skrample_amd.sampling import lazy
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    shape = (BATCH, *SHAPE)
    g = torch.Generator().manual_seed(1)
    fresh = lambda: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    result = {"form": form, "device": torch.cuda.get_device_name(0)}

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
        sample_numel = numel // BATCH
        for n in (3, 4):
            ops, cond = [fresh() for _ in range(n)], fresh()
            out, guided = torch.empty_like(cond), torch.empty_like(cond)
            factor = torch.empty(BATCH, dtype=torch.bfloat16, device=dev)
            plan = _hip.StepPlanC()
            plan.n_terms = plan.n_group_a = n
            plan.dtype_a = plan.out0_dtype = _hip.BF16
            plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
            for k in range(n):
                plan.coef0[k] = 0.5 - 0.1 * k

            def new_form():
                _hip.launch_guidance_factor(ops[1], cond, SCALE, sample_numel, factor)
                _hip.launch_step_guided_rescaled(plan, ops, out, cond, guided, SCALE, 1, factor, PHI, sample_numel, None, numel, dev)

            def torch_lines_and_step():
                _hip.launch_step(plan, [ops[0], torch_lines(ops[1], cond, SCALE, PHI), *ops[2:]], out, None, None, numel, dev)

            result[f"new{n}_us"] = timed(new_form)
            result[f"lines{n}_us"] = timed(torch_lines_and_step)
            if n == 3:
                result["stat_us"] = timed(lambda: _hip.launch_guidance_factor(ops[1], cond, SCALE, sample_numel, factor))
                result["stat_bytes"] = numel * 2 * 2
        print("RESULT " + json.dumps(result), flush=True)
        return

    if form == "r":
        for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
            same = samples = elements = differing = 0
            view = torch.int16 if dtype == torch.bfloat16 else torch.int32
            for seed in range(8):
                gen = torch.Generator().manual_seed(500 + seed)
                u, c = (torch.randn((8, 4, 32, 32), generator=gen).to(dtype).to(dev) for _ in range(2))
                p = u + SCALE * (c - u)
                theirs = (c.std(dim=[1, 2, 3], keepdim=True) / p.std(dim=[1, 2, 3], keepdim=True)).view(view)
                ours = lazy.Guidance(u, c, SCALE).factor().view(view)
                equal = (theirs == ours).flatten()
                same, samples = same + int(equal.sum()), samples + 8
                got, want = lazy.guide_only(lazy.Guidance(u, c, SCALE, PHI)).view(view), torch_lines(u, c, SCALE, PHI).view(view)
                off = (got != want).flatten(1).sum(1)
                assert int(off[equal].sum()) == 0, "a sample with torch's factor has torch's bits"
                elements, differing = elements + int((~equal).sum()) * u[0].numel(), differing + int(off.sum())
            result[name] = [same, samples, differing, elements]
        print("RESULT " + json.dumps(result), flush=True)
        return

    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    x0 = fresh()
    big = lambda: (torch.randn((2 * BATCH, *SHAPE), generator=g) * 0.1).bfloat16().to(dev)  # noqa: E731
    ring = [big().chunk(2) for _ in range(4)]  # (doubled-batch outputs: fresh memory to the history's alias guard, as a network's would be)

    if form in ("ln", "lo"):
        turn = itertools.count()

        def halves(x, t):  # the "network": the next pair of the ring (which pair a step reads is frozen into the graph)
            return ring[next(turn) & 3]

        if form == "ln":
            loop = capture_sampling_loop(w, halves, x0, steps, guidance_scale=SCALE, guidance_rescale=PHI)
        else:
            loop = capture_sampling_loop(w, lambda x, t: torch_lines(*halves(x, t), SCALE, PHI), x0, steps)
        for _ in range(2):
            loop(x0)
        torch.cuda.synchronize()
        event_us = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loop(x0)
            e1.record()
            torch.cuda.synchronize()
            event_us.append(e0.elapsed_time(e1) * 1e3 / steps)
        result.update(event_us=event_us)
        print("RESULT " + json.dumps(result), flush=True)
        return

    def run(ts):
        x = x0
        for i, t in enumerate(ts):
            uncond, cond = ring[i & 3]
            if form == "en":
                x = w.step_guided(uncond, cond, SCALE, t, x, return_dict=False, guidance_rescale=PHI)[0]
            else:
                x = w.step(torch_lines(uncond, cond, SCALE, PHI), t, x, return_dict=False)[0]
        return x

    def schedule():
        w.set_timesteps(steps)
        return w.timesteps.tolist()

    for _ in range(2):  # (two whole runs: the plain steps of form eo are served by the replayed fast path from the second run on)
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
    result.update(event_us=event_us, wall_us=wall_us)
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_rescale.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200:
        ap.error("at least 5 repeats of at least 200 steps")
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

    def judged(label, new, old):
        (nm, nlo, nhi), (om, olo, ohi) = summary(new), summary(old)
        margin = (nhi - nlo) + (ohi - olo)
        ok = om - nm > margin
        return ok, f"  {label}: yardstick - new = {om - nm:.2f} us (new / yardstick = {nm / om:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL (the new form is not below the yardstick by more than the spreads)'}"

    lines = [f"rescaled guidance: {BATCH} x {SHAPE} bf16 latents, DPM-2, guidance scale {SCALE}, guidance_rescale {PHI}, no network; {args.repeats} repeats of {args.steps} steps",
             "us per step: median (min - max) over the repeats, event clock unless stated; one child process per form"]  # fmt: skip
    failed = False
    k = spawn("k")
    if k is None:
        return 1
    lines.append(f"kernels alone, through the C ABI  ({k['device']})")
    for n in (3, 4):
        for name, what in (("new", "statistic + skr_step_launch_guided_rescaled"), ("lines", "torch's nine kernels + skr_step_launch")):
            m, lo, hi = summary(k[f"{name}{n}_us"])
            lines.append(f"  k  {what:44s} {n} operands   {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
        ok, text = judged(f"k  {n} operands, expected from {EXPECTED[n][0]} against {EXPECTED[n][1]} tensor passes: {EXPECTED[n][0] / EXPECTED[n][1]:.2f}", k[f"new{n}_us"], k[f"lines{n}_us"])
        failed |= not ok
        lines.append(text)
    m, lo, hi = summary(k["stat_us"])
    lines.append(f"  k  skr_guidance_rescale_factor alone            {m:8.2f} ({lo:8.2f} - {hi:8.2f})   {k['stat_bytes'] / 1e6:.1f} MB read -> {k['stat_bytes'] / (m * 1e-6) / PEAK * 100:.1f} % of 8 TB/s")
    seen = {}
    for form in FORMS:
        seen[form] = spawn(form)
        if seen[form] is None:
            return 1
    lines.append("a captured DPM-2 loop, indexed=False, replayed")
    for form in ("ln", "lo"):
        m, lo, hi = summary(seen[form]["event_us"])
        lines.append(f"  {form}  {FORMS[form]:38s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
    ok, text = judged("captured loop", seen["ln"]["event_us"], seen["lo"]["event_us"])
    failed |= not ok
    lines.append(text)
    lines.append("the eager wrapper call (host-bound; reported, not judged)")
    for form in ("en", "eo"):
        (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
        lines.append(f"  {form}  {FORMS[form]:38s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})")
    r = spawn("r")
    if r is None:
        return 1
    lines.append("for the record (not a promise: torch's device reduction order is not ours): the factor against the diffusers lines with torch's own device std")
    for name in ("bf16", "fp32"):
        same, samples, differing, elements = r[name]
        lines.append(f"  r  {name}: {same} of {samples} samples have the same factor; where it differs, {differing} of {elements} elements of the rescaled prediction differ")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
