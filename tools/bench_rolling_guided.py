"""Cost of one guided tick of a rolling batch (skrample_amd.rolling) against the unfused route, host side included: capacity 64 x
(4, 128, 128) bf16, classifier-free guidance with one scale, the two halves of the network output given (fixed tensors: no network is timed).

  python tools/bench_rolling_guided.py [--repeats 7] [--ticks 200] [--out profiles/rolling_guided.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  three torch lines + step()     noise_pred = uncond + g * (cond - uncond) on the whole batch, then RollingBatch.step(noise_pred): the
                                    yardstick, untouched code -- three elementwise kernels (8 tensor passes) and skr_step_launch_rolling
  b  step_guided(), 64 of 64        RollingBatch(guided=True).step_guided(uncond, cond): ONE skr_step_launch_guided_rolling
  c  step_guided(), 16 of 64        the same with every fourth slot resident: the other 48 samples' workgroups leave on their first scalar
                                    branch (for information: no condition attached)
  da / db                           forms a / b on a batch with device_positions=True: advance() in front of every tick, no host-to-device
                                    copy (the host-published tick of a / b / c copies its index and timesteps from pageable memory)
  ka / kb                           the device work of forms a / b alone: the three torch kernels and skr_step_launch_rolling, against
                                    skr_step_launch_guided_rolling, on steady-state rows (every operand present), 20 ticks captured in one
                                    graph and the graph replayed -- no host work between the kernels
Samplers: DPM-2 (eta = 0) and DPM-2 SDE (eta = 1, Random noise drawn in the kernel).  Every resident slot is admitted once with a run long
enough for the warm-up and all repeats, so no slot finishes inside a timed region.
Per repeat, `ticks` ticks are timed with HIP events (first enqueue to last kernel) and with the wall clock (first call to the end of a
device synchronisation); reported per form: median and min - max over the repeats, us per tick.
Pass condition, per sampler, pair (a / b, da / db, ka / kb) and clock: the guided form's median is below the yardstick's by more than the
two forms' min - max spreads put together."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, SHAPE, WARMUP, SCALE = 64, (4, 128, 128), 50, 7.5
SAMPLERS = {"dpm2": 0.0, "dpm2_sde": 1.0}
FORMS = {"a": "three torch lines + step()", "b": "step_guided(), 64 of 64", "c": "step_guided(), 16 of 64",
         "da": "device positions: a", "db": "device positions: b", "ka": "kernels alone: a", "kb": "kernels alone: b"}  # fmt: skip
PAIRS = (("a", "b"), ("da", "db"), ("ka", "kb"))
PER_GRAPH = 20  # ticks of a kernels-alone graph


def kernels_alone(batch, guided: bool, uncond, cond, repeats: int, ticks: int):
    """forms ka / kb: every slot on a steady-state row of its run (position 8 of 16: no operand absent), the tick's device work captured
    PER_GRAPH times over in one graph; returns (event us, wall us) per tick of every repeat"""
    import torch

    dev = batch.device
    batch.index_dev.copy_(torch.tensor([b * batch.max_steps + 8 for b in range(batch.capacity)], dtype=torch.int32))

    def work():  # (the eager tick's own binding, the rings left where they stand)
        for _ in range(PER_GRAPH):
            prediction = uncond if guided else uncond + SCALE * (cond - uncond)
            if guided:
                batch._launch(*batch._operands(prediction), cond, batch._g[0] if batch._g else None)
            else:
                batch._launch(*batch._operands(prediction))

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    replays = (ticks + PER_GRAPH - 1) // PER_GRAPH
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    event_us, wall_us = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        wall_us.append((time.perf_counter() - t0) * 1e6 / (replays * PER_GRAPH))
        event_us.append(e0.elapsed_time(e1) * 1e3 / (replays * PER_GRAPH))
    return event_us, wall_us


def child(form: str, sampler: str, repeats: int, ticks: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd.rolling import RollingBatch
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    eta = SAMPLERS[sampler]
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=eta), PS.Karras(PS.Scaled()))  # noqa: E731
    alone, on_device = form in ("ka", "kb"), form in ("da", "db")
    steps = 16 if alone else WARMUP + repeats * ticks + 8
    example = torch.zeros((CAPACITY, *SHAPE), dtype=torch.bfloat16, device=dev)
    guided = form not in ("a", "da", "ka")
    batch = RollingBatch(make, example, capacity=CAPACITY, max_steps=steps, guided=guided, device_positions=on_device)
    g = torch.Generator().manual_seed(1)
    uncond, cond = (torch.randn((CAPACITY, *SHAPE), generator=g).bfloat16().to(dev) for _ in range(2))

    def tick():
        if on_device:
            batch.advance()
        return batch.step_guided(uncond, cond) if guided else batch.step(uncond + SCALE * (cond - uncond))

    resident = [slot for slot in range(CAPACITY) if form != "c" or slot % 4 == 0]
    for slot in resident:
        batch.admit(slot, torch.randn(SHAPE, generator=g).bfloat16().to(dev), make(), steps, seed=slot + 1 if eta else None, **(dict(guidance_scale=SCALE) if guided else {}))
    if alone:
        event_us, wall_us = kernels_alone(batch, guided, uncond, cond, repeats, ticks)
        print("RESULT " + json.dumps({"form": form, "sampler": sampler, "event_us": event_us, "wall_us": wall_us, "device": torch.cuda.get_device_name(0)}), flush=True)
        return
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
    assert len(batch.active) == len(resident)  # nothing finished inside the timed regions
    print("RESULT " + json.dumps({"form": form, "sampler": sampler, "event_us": event_us, "wall_us": wall_us, "device": torch.cuda.get_device_name(0)}), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_guided.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    args = ap.parse_args()
    if args.repeats < 7 or args.ticks < 200:
        ap.error("at least 7 repeats of at least 200 ticks")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.ticks)
        return 0
    lines = [f"guided rolling ticks: capacity {CAPACITY} x {SHAPE} bf16, guidance scale {SCALE}, fixed uncond / cond tensors (no network); {args.repeats} repeats of "
             f"{args.ticks} ticks after {WARMUP} warm-up ticks",
             "us per tick: median (min - max) over the repeats; one child process per form and sampler",
             "tensor passes per tick over N = capacity x sample elements: a 8 N (three torch kernels) + 4 N (step: x, noise_pred, one history in; out) = 12 N;  "
             "b 6 N (x, uncond, cond, one history in; out, guided_out)"]  # fmt: skip
    failed = False
    for sampler in SAMPLERS:
        seen = {}
        for form in FORMS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--ticks", str(args.ticks), "--child", form, sampler],
                                 capture_output=True, text=True, timeout=420)  # fmt: skip
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"form {form} / {sampler} failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[form] = json.loads(found[-1][len("RESULT "):])
            print(f"[{sampler} / {form}] done", file=sys.stderr, flush=True)
        lines.append(f"{sampler}  ({seen['a']['device']})")
        for form, what in FORMS.items():
            (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
            lines.append(f"  {form}  {what:28s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})")
        for first, second in PAIRS:
            for clock in ("event_us", "wall_us"):
                (am, alo, ahi), (bm, blo, bhi) = summary(seen[first][clock]), summary(seen[second][clock])
                margin = (ahi - alo) + (bhi - blo)
                ok = am - bm > margin
                failed |= not ok
                lines.append(f"  {clock[:-3]}-clock medians: {first} - {second} = {am - bm:.2f} us ({second} is {bm / am:.2f} of {first}), the two spreads together {margin:.2f} us: "
                             f"{'PASS' if ok else 'FAIL'} ({second} below {first} by more than the spreads)")  # fmt: skip
        cm, bm = summary(seen["c"]["event_us"])[0], summary(seen["b"]["event_us"])[0]
        lines.append(f"  for information: c is {cm / bm:.2f} of b on the event clock with a quarter of the slots resident")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
