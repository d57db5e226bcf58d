"""Cost of one rescaled guided tick of a rolling batch (skrample_amd.rolling) against what a server runs without it: capacity 64 x
(4, 128, 128) bf16, guidance scale 7.5, guidance_rescale 0.7, the two halves of the network output given (fixed tensors: no network is timed).

  python tools/bench_rolling_guided_rescale.py [--repeats 7] [--ticks 200] [--out profiles/rolling_guided_rescale.txt]

Forms, each in a child process of its own under its own time limit (a fresh HIP context and allocator per form; the parent never opens the
GPU; nothing more is started after a form fails):
  ka / kb   JUDGED.  The device work of a tick alone, on steady-state rows (every operand present), 20 ticks captured in one graph and the
            graph replayed.  ka, the yardstick, measured in the same run: diffusers' lines by torch on the whole batch -- three guidance
            kernels, two whole-sample std reductions, the division of the two (capacity elements) and four elementwise kernels -- and
            skr_step_launch_rolling of a plain batch.  kb: skr_guidance_rescale_factor_rolling + skr_step_launch_guided_rescaled_rolling.
  da / db   reported: the tick with device_positions=True (advance() in front), yardstick / RollingBatch(guided=True, rescaled=True)
  a / b     reported: the host-published tick.  It is host-bound (DESIGN.md section 4.7 "Rolling batches" (c)): two copies from pageable
            memory and per-slot Python bookkeeping hide the device time of either form.
  sa .. sd  reported: the statistics launch alone, 20 in one replayed graph.  sa: skr_guidance_rescale_factor on the whole batch;
            sb: skr_guidance_rescale_factor_rolling, 64 of 64 slots active and rescaling (the expected difference is the one dependent
            scalar round trip per workgroup; DESIGN.md section 8 measured 0.77 us for the like); sc: 16 of 64 slots rescaling, the others
            phi = 0; sd: 16 of 64 slots active -- whether the early exits are visible at this size.
Samplers: DPM-2 (eta = 0) and DPM-2 SDE (eta = 1, Random noise drawn in the kernel); the statistics forms do not depend on the sampler
and run once.  Per repeat, `ticks` ticks are timed with HIP events; reported per form: median and min - max over the repeats, us per tick.

Expectation, written before the run: for DPM-2 the yardstick makes 23 tensor passes over N = capacity x sample elements (8 N the three
guidance kernels, 2 N the two reductions, 9 N the four elementwise kernels, 4 N the step) where the two launches make 8 N (2 N the
statistic, 6 N the step).  The eager measurement at 256 samples gave 0.34 (profiles/guided_rescale.txt).  This benchmark's tensors fit
the Infinity Cache and the statistics launch is bound by fp64 issue, not by bytes (27 us at 256 samples), so no ratio is fixed in advance.
Pass condition (ka / kb, per sampler): kb's median is below ka's by more than the two forms' min - max spreads put together."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, SHAPE, WARMUP, SCALE, PHI = 64, (4, 128, 128), 50, 7.5, 0.7
SAMPLERS = {"dpm2": 0.0, "dpm2_sde": 1.0}
FORMS = {"ka": "kernels alone: torch's lines + rolling step", "kb": "kernels alone: the two launches", "da": "device positions: yardstick",
         "db": "device positions: rescaled batch", "a": "host-published: yardstick", "b": "host-published: rescaled batch"}  # fmt: skip
STAT_FORMS = {"sa": "whole-batch statistics launch", "sb": "rolling, 64 of 64 rescaling", "sc": "rolling, 16 of 64 rescaling", "sd": "rolling, 16 of 64 active"}
PER_GRAPH = 20  # launches of a kernels-alone graph
LIMIT = 420  # seconds a child may take


def torch_lines(uncond, cond):
    "diffusers' three guidance lines and rescale_noise_cfg, by torch on the whole batch"
    p = uncond + SCALE * (cond - uncond)
    dims = list(range(1, cond.ndim))
    resc = p * (cond.std(dim=dims, keepdim=True) / p.std(dim=dims, keepdim=True))
    return PHI * resc + (1 - PHI) * p


def replayed(work, dev, repeats: int, ticks: int):
    "`work` (PER_GRAPH ticks of device work) captured in one graph; event us per tick of every repeat"
    import torch

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
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        event_us.append(e0.elapsed_time(e1) * 1e3 / (replays * PER_GRAPH))
    return event_us


def child(form: str, sampler: str, repeats: int, ticks: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.rolling import RollingBatch
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    eta = SAMPLERS[sampler]
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=eta), PS.Karras(PS.Scaled()))  # noqa: E731
    alone, on_device = form[0] in "ks", form in ("da", "db")
    steps = 16 if alone else WARMUP + repeats * ticks + 8
    example = torch.zeros((CAPACITY, *SHAPE), dtype=torch.bfloat16, device=dev)
    rescaled = form not in ("a", "da", "ka")
    batch = RollingBatch(make, example, capacity=CAPACITY, max_steps=steps, guided=rescaled, rescaled=rescaled, device_positions=on_device)
    g = torch.Generator().manual_seed(1)
    uncond, cond = (torch.randn((CAPACITY, *SHAPE), generator=g).bfloat16().to(dev) for _ in range(2))
    resident = [slot for slot in range(CAPACITY) if form != "sd" or slot % 4 == 0]
    for slot in resident:
        phi = 0.0 if form == "sc" and slot % 4 else PHI
        extra = dict(guidance_scale=SCALE, guidance_rescale=phi) if rescaled else {}
        batch.admit(slot, torch.randn(SHAPE, generator=g).bfloat16().to(dev), make(), steps, seed=slot + 1 if eta else None, **extra)
    result = {"form": form, "sampler": sampler, "device": torch.cuda.get_device_name(0)}
    if alone:
        # every resident slot on a steady-state row of its run (position 8 of 16: no operand absent)
        batch.index_dev.copy_(torch.tensor([b * batch.max_steps + 8 if b in resident else -1 for b in range(CAPACITY)], dtype=torch.int32))
        lib = _hip.load()

        def work():
            for _ in range(PER_GRAPH):
                stream = _hip.current_stream_ptr(dev)
                if form == "sa":
                    status = lib.skr_guidance_rescale_factor(uncond.data_ptr(), cond.data_ptr(), _hip.BF16, SCALE, batch.numel, batch.sample_numel, batch.factor.data_ptr(), None,
                                                             batch._partials.data_ptr(), stream)  # fmt: skip
                    _hip.check(status, "skr_guidance_rescale_factor")
                elif form[0] == "s":
                    status = lib.skr_guidance_rescale_factor_rolling(uncond.data_ptr(), cond.data_ptr(), _hip.BF16, batch.numel, batch.sample_numel, batch.rows_dev.data_ptr(),
                                                                     batch.index_dev.data_ptr(), 0, batch.factor.data_ptr(), None, batch._partials.data_ptr(), stream)  # fmt: skip
                    _hip.check(status, "skr_guidance_rescale_factor_rolling")
                else:
                    prediction = uncond if rescaled else torch_lines(uncond, cond)
                    if rescaled:  # (the eager tick's own binding, the rings left where they stand)
                        batch._launch(*batch._operands(prediction), cond, batch._g[0] if batch._g else None)
                    else:
                        batch._launch(*batch._operands(prediction))

        result["event_us"] = replayed(work, dev, repeats, ticks)
        print("RESULT " + json.dumps(result), flush=True)
        return

    def tick():
        if on_device:
            batch.advance()
        return batch.step_guided(uncond, cond) if rescaled else batch.step(torch_lines(uncond, cond))

    for _ in range(WARMUP):
        tick()
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ticks):
            tick()
        e1.record()
        torch.cuda.synchronize()
        event_us.append(e0.elapsed_time(e1) * 1e3 / ticks)
    assert len(batch.active) == len(resident)  # nothing finished inside the timed regions
    result["event_us"] = event_us
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_guided_rescale.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    args = ap.parse_args()
    if args.repeats < 7 or args.ticks < 200:
        ap.error("at least 7 repeats of at least 200 ticks")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.ticks)
        return 0
    lines = [f"rescaled guided rolling ticks: capacity {CAPACITY} x {SHAPE} bf16, guidance scale {SCALE}, guidance_rescale {PHI}, fixed uncond / cond tensors (no network); "
             f"{args.repeats} repeats of {args.ticks} ticks, event clock",
             "us per tick: median (min - max) over the repeats; one child process per form and sampler",
             "tensor passes per tick over N = capacity x sample elements (DPM-2): yardstick 8 N (three guidance kernels) + 2 N (two std reductions) + 9 N (four elementwise "
             "kernels) + 4 N (step) = 23 N;  the two launches 2 N (statistic: uncond, cond) + 6 N (step: x, uncond, cond, one history in; out, guided_out) = 8 N",
             "expectation, written before the run: no ratio fixed in advance (the tensors fit the Infinity Cache; the statistics launch is bound by fp64 issue)"]  # fmt: skip
    failed = False

    def run(form, sampler):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--ticks", str(args.ticks), "--child", form, sampler],
                              capture_output=True, text=True, timeout=LIMIT)  # fmt: skip
        found = [line for line in done.stdout.splitlines() if line.startswith("RESULT ")]
        if done.returncode != 0 or not found:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            print(f"form {form} / {sampler} failed with exit status {done.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        print(f"[{sampler} / {form}] done", file=sys.stderr, flush=True)
        return json.loads(found[-1][len("RESULT "):])

    def row(form, what, seen):
        m, lo, hi = summary(seen["event_us"])
        return f"  {form:2s}  {what:46s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})"

    for sampler in SAMPLERS:
        seen = {}
        for form in FORMS:
            seen[form] = run(form, sampler)
            if seen[form] is None:
                return 1
        lines.append(f"{sampler}  ({seen['ka']['device']})")
        lines += [row(form, what, seen[form]) for form, what in FORMS.items()]
        for first, second, judged in (("ka", "kb", True), ("da", "db", False), ("a", "b", False)):
            (am, alo, ahi), (bm, blo, bhi) = summary(seen[first]["event_us"]), summary(seen[second]["event_us"])
            margin = (ahi - alo) + (bhi - blo)
            ok = am - bm > margin
            verdict = f"{'PASS' if ok else 'FAIL'} ({second} below {first} by more than the spreads)" if judged else "reported, not judged"
            failed |= judged and not ok
            lines.append(f"  medians: {first} - {second} = {am - bm:.2f} us ({second} is {bm / am:.2f} of {first}), the two spreads together {margin:.2f} us: {verdict}")
    seen = {}
    for form in STAT_FORMS:
        seen[form] = run(form, "dpm2")
        if seen[form] is None:
            return 1
    lines.append("the statistics launch alone (reported)")
    lines += [row(form, what, seen[form]) for form, what in STAT_FORMS.items()]
    medians = {form: summary(seen[form]["event_us"])[0] for form in STAT_FORMS}
    lines.append(f"  sb - sa = {medians['sb'] - medians['sa']:.2f} us;  sc is {medians['sc'] / medians['sb']:.2f} of sb;  sd is {medians['sd'] / medians['sb']:.2f} of sb")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
