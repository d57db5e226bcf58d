"""Cost of one tick of a rolling batch (skrample_amd.rolling), host side included: capacity 64 x (4, 128, 128) bf16, every slot resident,
the elementwise `net` of tests/test_rolling_gpu.py as the network.

  python tools/bench_rolling_ticks.py [--repeats 5] [--ticks 200] [--out profiles/rolling_ticks.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  host-published tick       RollingBatch(device_positions=False): step(net(latents, timesteps)) -- index and timesteps copied from
                               pageable host memory every tick
  b  device positions, eager   advance(); step(net(latents, timesteps)) -- no host-to-device copy, the network still eager
  c  captured ticks            CapturedTicks.tick(): one graph replay (advance + network) and one step launch
Samplers: DPM-2 (eta = 0) and UniPC-3.  Every slot is admitted once with a run long enough for the warm-up and all repeats, so no slot
finishes inside a timed region.  Per repeat, `ticks` ticks are timed with HIP events (first enqueue to last kernel) and with the wall
clock (first call to the end of a device synchronisation); reported per form: median and min - max over the repeats, us per tick.
Pass condition: c's wall-clock median is below a's by more than the two forms' min - max spreads put together."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, SHAPE, WARMUP = 64, (4, 128, 128), 50
SAMPLERS = ("dpm2", "unipc3")
FORMS = {"a": "host-published tick", "b": "device positions, eager", "c": "captured ticks"}


def net(x, t):
    return x * 0.5 + 0.3 * x.abs()


def child(form: str, sampler: str, repeats: int, ticks: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd.rolling import RollingBatch
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    make = (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))) if sampler == "dpm2" else (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3), PS.Karras(PS.Scaled())))  # fmt: skip
    steps = WARMUP + repeats * ticks + 8
    example = torch.zeros((CAPACITY, *SHAPE), dtype=torch.bfloat16, device=dev)
    batch = RollingBatch(make, example, capacity=CAPACITY, max_steps=steps, device_positions=form != "a")
    if form == "c":
        captured = batch.capture(net)
        tick = captured.tick
    elif form == "b":

        def tick():
            batch.advance()
            return batch.step(net(batch.latents, batch.timesteps))
    else:

        def tick():
            return batch.step(net(batch.latents, batch.timesteps))

    g = torch.Generator().manual_seed(1)
    for slot in range(CAPACITY):
        batch.admit(slot, torch.randn(SHAPE, generator=g).bfloat16().to(dev), make(), steps)
    for _ in range(WARMUP):
        tick()
    torch.cuda.synchronize()
    event_us, wall_us = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(ticks):
            tick()
        e1.record()
        torch.cuda.synchronize()
        wall_us.append((time.perf_counter() - t0) * 1e6 / ticks)
        event_us.append(e0.elapsed_time(e1) * 1e3 / ticks)
    assert len(batch.active) == CAPACITY  # nothing finished inside the timed regions
    print("RESULT " + json.dumps({"form": form, "sampler": sampler, "event_us": event_us, "wall_us": wall_us, "device": torch.cuda.get_device_name(0)}), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_ticks.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    args = ap.parse_args()
    if args.repeats < 5 or args.ticks < 200:
        ap.error("at least 5 repeats of at least 200 ticks")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.ticks)
        return 0
    lines = [f"rolling ticks: capacity {CAPACITY} x {SHAPE} bf16, all slots resident, elementwise net; {args.repeats} repeats of {args.ticks} ticks after {WARMUP} warm-up ticks",
             "us per tick: median (min - max) over the repeats; one child process per form and sampler"]  # fmt: skip
    failed = False
    for sampler in SAMPLERS:
        seen = {}
        for form in FORMS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--ticks", str(args.ticks), "--child", form, sampler],
                                 capture_output=True, text=True, timeout=600)  # fmt: skip
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"form {form} / {sampler} failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[form] = json.loads(found[-1][len("RESULT "):])
        lines.append(f"{sampler}  ({seen['a']['device']})")
        for form, what in FORMS.items():
            (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
            lines.append(f"  {form}  {what:26s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})")
        (am, alo, ahi), (cm, clo, chi) = summary(seen["a"]["wall_us"]), summary(seen["c"]["wall_us"])
        margin = (ahi - alo) + (chi - clo)
        ok = am - cm > margin
        failed |= not ok
        lines.append(f"  wall-clock medians: a - c = {am - cm:.2f} us, the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (c below a by more than the spreads)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
