"""Cost of adaptive projected guidance: the eager DPM-2 step_guided() loop under set_projected_guidance(eta=0, norm_threshold=r,
momentum=-0.5) against what a pipeline runs today -- the APG lines in torch (running average, per-sample norm and clamp, the projection
onto cond on tensors widened to float64, the guided sum) and then the same wrapper's step().  bf16 latents, no network (a ring of fixed
halves), at 64 x (4, 128, 128) and 64 x (3, 64, 64).

  python tools/bench_projected_guidance.py [--rounds 3] [--repeats 5] [--steps 200] [--out profiles/projected_guidance.txt]

The two routes alternate, each run in a child process of its own (a fresh HIP context and allocator; the parent never opens the GPU):
`rounds` times new, old, new, old ...  Per child `repeats` runs of `steps` steps are timed with HIP events (first enqueue to last kernel)
and with the wall clock (to the end of a device synchronisation); reported per route and size: median and min - max over every repeat of
every round, us per step.  A speed-up is claimed only where the yardstick's median exceeds the new route's by more than the two min - max
spreads together; otherwise the line says so.  The statistics launch alone is timed through the C ABI beside its byte count (three
tensor reads and one write with momentum).
Tensor passes expected from the definition, a DPM-2 middle step, with momentum: statistic 3 reads + 1 write, step 2 + 5 reads + 2 writes
(13) against about twenty passes of torch lines, several at 8 bytes an element, plus the step's 7."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = {"4x128x128": (64, 4, 128, 128), "3x64x64": (64, 3, 64, 64)}
WARMUP_RUNS, SCALE, ETA, BETA = 2, 7.5, 0.0, -0.5
PEAK = 8.0e12  # bytes per second


def apg_lines(u, c, scale, eta, r, beta, state):
    "the pipeline's lines: momentum, norm clamp, projection on float64 tensors, guided sum"
    dims = list(range(1, c.ndim))
    diff = c - u
    if beta != 0.0:
        state["m"] = diff = diff + beta * state["m"]
    if r > 0.0:
        norm = diff.norm(p=2, dim=dims, keepdim=True)
        diff = diff * torch_minimum_one(r / norm)
    v0, v1 = diff.double(), c.double()
    v1 = v1 / v1.norm(p=2, dim=dims, keepdim=True).clamp_min(1e-12)
    par = (v0 * v1).sum(dim=dims, keepdim=True) * v1
    orth = v0 - par
    update = orth.to(c.dtype) + eta * par.to(c.dtype)
    return c + (scale - 1.0) * update


def torch_minimum_one(t):
    import torch

    return torch.minimum(torch.ones_like(t), t)


def child(form: str, size: str, repeats: int, steps: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.sampling import structured as PT

    dev, shape = torch.device("cuda:0"), SIZES[size]
    g = torch.Generator().manual_seed(1)
    fresh = lambda: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    ring = [(fresh(), fresh()) for _ in range(4)]
    x0 = fresh()
    r = 0.5 * float((ring[0][1].double() - ring[0][0].double()).reshape(shape[0], -1).norm(dim=1).mean())  # a threshold that clamps
    result = {"form": form, "size": size, "device": torch.cuda.get_device_name(0)}

    if form == "stat":
        u, c = ring[0]
        m, numel, sample_numel = torch.zeros_like(u), u.numel(), u.numel() // shape[0]
        coef = torch.empty(2 * shape[0], dtype=torch.float32, device=dev)
        partials = torch.empty(_hip.projected_partials(numel, sample_numel), dtype=torch.float64, device=dev)
        launch = lambda: _hip.launch_projected_coef(u, c, m, SCALE, ETA, r, BETA, sample_numel, coef, partials)  # noqa: E731
        for _ in range(50):
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
        result.update(event_us=per, bytes=numel * 2 * 4)
        print("RESULT " + json.dumps(result), flush=True)
        return

    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    if form == "new":
        w.set_projected_guidance(eta=ETA, norm_threshold=r, momentum=BETA)

    def run(ts):
        x, state = x0, {"m": torch.zeros_like(x0)}
        for i, t in enumerate(ts):
            u, c = ring[i & 3]
            if form == "new":
                x = w.step_guided(u, c, SCALE, t, x, return_dict=False)[0]
            else:
                x = w.step(apg_lines(u, c, SCALE, ETA, r, BETA, state), t, x, return_dict=False)[0]
        return x

    def schedule():
        w.set_timesteps(steps)
        return w.timesteps.tolist()

    for _ in range(WARMUP_RUNS):  # (whole runs: the plain steps of the yardstick are served by the replayed fast path from the second run on)
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projected_guidance.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SIZE"))
    args = ap.parse_args()
    if args.child:
        child(*args.child, args.repeats, args.steps)
        return 0

    def spawn(form, size):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--child", form, size],
                             capture_output=True, text=True, timeout=300)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} at {size} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        return json.loads(found[-1][len("RESULT "):])

    lines = [f"adaptive projected guidance: eager DPM-2 loop, bf16, guidance scale {SCALE}, eta {ETA}, momentum {BETA}, a threshold that clamps, no network; "
             f"{args.rounds} alternating rounds of {args.repeats} repeats of {args.steps} steps, one child process per route and round",
             "us per step: median (min - max) over all repeats"]  # fmt: skip
    for size in SIZES:
        seen = {"new": {"event_us": [], "wall_us": []}, "old": {"event_us": [], "wall_us": []}}
        for _ in range(args.rounds):
            for form in ("new", "old"):
                got = spawn(form, size)
                if got is None:
                    return 1
                seen[form]["event_us"] += got["event_us"]
                seen[form]["wall_us"] += got["wall_us"]
        lines.append(f"64 x {size}  ({got['device']})")
        for form, what in (("new", "step_guided under set_projected_guidance"), ("old", "torch APG lines (fp64 projection) + step()")):
            (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
            lines.append(f"  {form}  {what:44s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})")
        (nm, nlo, nhi), (om, olo, ohi) = summary(seen["new"]["event_us"]), summary(seen["old"]["event_us"])
        margin = (nhi - nlo) + (ohi - olo)
        verdict = f"faster: new / old = {nm / om:.2f}" if om - nm > margin else "NO speed-up claimed: the difference does not exceed the spreads"
        lines.append(f"  old - new = {om - nm:.2f} us, the two spreads together {margin:.2f} us: {verdict}")
        stat = spawn("stat", size)
        if stat is None:
            return 1
        m, lo, hi = summary(stat["event_us"])
        lines.append(f"  skr_projected_guidance_coef alone (momentum)    {m:8.2f} ({lo:8.2f} - {hi:8.2f})   {stat['bytes'] / 1e6:.1f} MB moved -> {stat['bytes'] / (m * 1e-6) / PEAK * 100:.1f} % of 8 TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
