"""Cost of one tick of a rolling batch whose requests are in-painting ones: the masked rolling launch against what a server does without it.
Capacity 64 x (4, 128, 128) bf16 with a (1, 128, 128) bf16 mask per slot, every slot resident and in-painting, the elementwise `net` of
tests/test_rolling_gpu.py as the network; DPM-2 (eta = 0 and eta = 1) and Euler.

  python tools/bench_masked_rolling.py [--repeats 5] [--ticks 200] [--out profiles/masked_rolling.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  masked rolling tick    RollingBatch(inpaint_mask_shape=...), admit(..., inpaint=(mask, original, noise)):
                            step(net(latents, timesteps)) -- ONE skr_step_launch_masked_rolling
  b  plain tick + torch     a plain RollingBatch tick (skr_step_launch_rolling), then the re-noising and the blend with torch elementwise
                            kernels: every slot's alpha and sigma of its NEXT schedule point in one [2, B, 1, 1, 1] device tensor uploaded
                            per tick, latents.copy_(mask * latents + (1 - mask) * (alpha * original + sigma * noise)), 1 - mask precomputed
  k  kernels alone          skr_step_launch_masked_rolling back to back on full rows of the tick's operand count, beside
                            skr_step_launch_masked_indexed_per_sample (masked_kernel_v1<..., PerSample>) on the same rows: event clock
                            per launch and the fraction of 8 TB/s its algorithmic bytes come to (operands + quarter-size mask + one store)
Every slot is admitted once with a run long enough for the warm-up and all repeats, so no slot finishes inside a timed region.  Per
repeat, `ticks` ticks are timed with HIP events (first enqueue to last kernel) and with the wall clock (first call to the end of a device
synchronisation); reported per form: median and min - max over the repeats, us per tick.
Pass condition: a's wall-clock median is below b's by more than the two forms' min - max spreads put together."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, SHAPE, MASK, WARMUP = 64, (4, 128, 128), (1, 128, 128), 50
SAMPLERS = {"dpm2": "DPM-2, eta = 0", "dpm2_sde": "DPM-2, eta = 1", "euler": "Euler"}
FORMS = {"a": "masked rolling tick", "b": "plain tick + torch blend"}
PEAK = 8.0e12  # bytes per second


def net(x, t):
    return x * 0.5 + 0.3 * x.abs()


def child(form: str, sampler: str, repeats: int, ticks: int) -> None:
    import ctypes

    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.rolling import RollingBatch
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    samplers = {"dpm2": lambda: PT.DPM(order=2), "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1.0), "euler": lambda: PT.Euler()}
    make = lambda: PD.SkrampleWrapperScheduler(samplers[sampler](), PS.Karras(PS.Scaled()))  # noqa: E731
    noisy = sampler == "dpm2_sde"
    g = torch.Generator().manual_seed(1)
    fresh = lambda shape: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    example = torch.zeros((CAPACITY, *SHAPE), dtype=torch.bfloat16, device=dev)
    result = {"form": form, "sampler": sampler, "device": torch.cuda.get_device_name(0)}

    if form == "k":
        n = RollingBatch(make, example[:1], capacity=1, inpaint_mask_shape=MASK).plan.n_terms  # the tick's operand count
        ops = [fresh((CAPACITY, *SHAPE)) for _ in range(n)]
        mask = torch.rand((CAPACITY, *MASK), generator=g).bfloat16().to(dev)
        out = torch.empty_like(example)
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = n
        plan.dtype_a = plan.out0_dtype = _hip.BF16
        plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
        plan.sample_numel, plan.noise_mode = example[0].numel(), 1 if noisy else 0
        row = _hip.StepRowC()
        for k in range(n):
            row.coef0[k] = 0.5 if k < n - 2 else 0.0
            row.coef1[k] = 0.5 if k >= n - 2 else 0.0
        row.zeta0, row.stream0 = (0.3, 256) if noisy else (0.0, 0)
        table = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
        _hip.upload_rows(table, 0, [row])
        index = torch.zeros(CAPACITY, dtype=torch.int32, device=dev)
        seeds = torch.arange(1, CAPACITY + 1, dtype=torch.int64, device=dev)
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ops])
        per_sample = mask.numel() // CAPACITY
        desc = _hip.StepMaskC(mask.data_ptr(), _hip.BF16, 0, per_sample, per_sample)
        lib = _hip.load()
        for name, entry in (("rolling", lib.skr_step_launch_masked_rolling), ("rows", lib.skr_step_launch_masked_indexed_per_sample)):

            def launch():
                _hip.check(entry(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), seeds.data_ptr() if noisy else None, out.numel(), table.data_ptr(),
                                 index.data_ptr(), 0, _hip.current_stream_ptr(dev)), name)  # fmt: skip

            for _ in range(WARMUP):
                launch()
            torch.cuda.synchronize()
            per = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(ticks):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / ticks)
            result[name + "_us"] = per
        result["operands"] = n
        result["bytes"] = out.numel() * 2 * (n + 1) + mask.numel() * 2
        print("RESULT " + json.dumps(result), flush=True)
        return

    steps = WARMUP + repeats * ticks + 8
    batch = RollingBatch(make, example, capacity=CAPACITY, max_steps=steps, inpaint_mask_shape=MASK if form == "a" else None)
    masks = torch.rand((CAPACITY, *MASK), generator=g).bfloat16().to(dev)
    original, noise = fresh((CAPACITY, *SHAPE)), fresh((CAPACITY, *SHAPE))
    levels = []  # form b: (alpha, sigma) of every slot's schedule points, on the host
    for slot in range(CAPACITY):
        w = make()
        inpaint = (masks[slot], original[slot], noise[slot]) if form == "a" else None
        batch.admit(slot, fresh(SHAPE), w, steps, seed=slot + 1 if noisy else None, inpaint=inpaint)
        points = w.schedule_np
        levels.append(([float(p[2]) for p in points[1:]] + [1.0], [float(p[1]) for p in points[1:]] + [0.0]))

    if form == "a":

        def tick():
            return batch.step(net(batch.latents, batch.timesteps))
    else:
        masks4, inverse, position = masks, 1 - masks, [0] * CAPACITY  # (CAPACITY, 1, H, W): broadcast over the channels

        def tick():
            done = batch.step(net(batch.latents, batch.timesteps))
            both = torch.tensor([[levels[b][0][position[b]] for b in range(CAPACITY)], [levels[b][1][position[b]] for b in range(CAPACITY)]], dtype=torch.bfloat16)
            both = both.to(dev).reshape(2, CAPACITY, 1, 1, 1)
            x = batch.latents
            x.copy_(masks4 * x + inverse * (both[0] * original + both[1] * noise))
            for b in range(CAPACITY):
                position[b] += 1
            return done

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
    assert bool(torch.isfinite(batch.latents.float()).all())
    result.update(event_us=event_us, wall_us=wall_us, operands=batch.plan.n_terms)
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_rolling.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    args = ap.parse_args()
    if args.repeats < 5 or args.ticks < 200:
        ap.error("at least 5 repeats of at least 200 ticks")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.ticks)
        return 0
    lines = [f"masked rolling ticks: capacity {CAPACITY} x {SHAPE} bf16, a {MASK} bf16 mask per slot, all slots resident and in-painting, elementwise net; "
             f"{args.repeats} repeats of {args.ticks} ticks after {WARMUP} warm-up ticks",
             "us per tick: median (min - max) over the repeats; one child process per form and sampler"]  # fmt: skip
    failed = False
    for sampler, what in SAMPLERS.items():
        seen = {}
        for form in (*FORMS, "k"):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--ticks", str(args.ticks), "--child", form, sampler],
                                 capture_output=True, text=True, timeout=600)  # fmt: skip
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"form {form} / {sampler} failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[form] = json.loads(found[-1][len("RESULT "):])
        lines.append(f"{sampler}  ({what}; {seen['a']['device']})")
        for form, name in FORMS.items():
            (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
            lines.append(f"  {form}  {name:26s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})   step operands {seen[form]['operands']}")
        (am, alo, ahi), (bm, blo, bhi) = summary(seen["a"]["wall_us"]), summary(seen["b"]["wall_us"])
        margin = (ahi - alo) + (bhi - blo)
        ok = bm - am > margin
        failed |= not ok
        lines.append(f"  wall-clock medians: b - a = {bm - am:.2f} us (b / a = {bm / am:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (a below b by more than the spreads)")
        (eam, _, _), (ebm, _, _) = summary(seen["a"]["event_us"]), summary(seen["b"]["event_us"])
        lines.append(f"  event-clock medians: b / a = {ebm / eam:.2f}")
        k = seen["k"]
        for name, kernel in (("rolling", "masked_kernel_v1<..., Rolling>"), ("rows", "masked_kernel_v1<..., PerSample>")):
            m, lo, hi = summary(k[name + "_us"])
            lines.append(f"  k  {kernel:32s} {k['operands']} operands   event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f}) per launch   {k['bytes'] / 1e6:6.1f} MB -> {k['bytes'] / (m * 1e-6) / PEAK * 100:5.1f} % of 8 TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
