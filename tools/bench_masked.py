"""Cost of an in-painting step: the masked step() of SkrampleWrapperScheduler.set_inpaint against the loop it replaces.
256 x (4, 128, 128) bf16 latents, a (B, 1, H, W) bf16 mask, DPM-2 (eta = 0) and Euler, no network (a ring of fixed model outputs).

  python tools/bench_masked.py [--repeats 5] [--steps 200] [--out profiles/masked_step.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  masked step       w.set_inpaint(mask, original, noise);  latents = w.step(out, t, latents)
  b  unfused loop      latents = w.step(out, t, latents);  known = w.add_noise(original, noise, next t);
                       latents = mask * latents + (1 - mask) * known      -- the public API without set_inpaint
  c  captured loop     w.set_inpaint(...);  loop = capture_sampling_loop(w, model, latents, steps, indexed=True);  loop(latents)
                       -- the masked steps as skr_step_launch_masked_indexed launches of one HIP graph (device-resident rows); a replay
                       includes the copy of the latents into the loop's static buffer and the clone of its result
  k  kernels alone     skr_step_launch_masked back to back, beside skr_step_launch of the same operand count and beside
                       skr_step_launch_masked_indexed reading the same scalars from a row: event clock per launch and
                       the fraction of 8 TB/s its algorithmic bytes come to (operands + quarter-size mask + one store)
Per repeat, `steps` steps of a `steps`-step schedule are timed with HIP events (first enqueue to last kernel) and with the wall clock
(first call to the end of a device synchronisation); reported per form: median and min - max over the repeats, us per step.
Pass conditions: a's wall-clock median is below b's, and c's below a's, each by more than the two forms' min - max spreads put together.
Reported beside them, not judged: whether the row kernel's median lies within the min - max spread of its kernarg twin."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, WARMUP = 256, (4, 128, 128), 20
SAMPLERS = ("dpm2", "euler")
FORMS = {"a": "masked step()", "b": "step + add_noise + blend", "c": "indexed captured loop"}
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
    x0, orig, nz = fresh(), fresh(), fresh()
    ring = [fresh() * 0.1 for _ in range(4)]  # (model outputs: fresh memory to the history's alias guard, as a network's would be)
    mask = (torch.rand((BATCH, 1, *SHAPE[1:]), generator=g) < 0.5).bfloat16().to(dev)
    result = {"form": form, "sampler": sampler, "device": torch.cuda.get_device_name(0)}

    if form == "k":
        n = 5 if sampler == "dpm2" else 4  # sample, model output (, previous output), original, noise
        ops = [fresh() for _ in range(n)]
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = n
        plan.dtype_a = plan.out0_dtype = _hip.BF16
        plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
        plan.sample_numel = x0[0].numel()
        for k in range(n):
            plan.coef0[k] = 0.5 if k < n - 2 else 0.0
            plan.coef1[k] = 0.5 if k >= n - 2 else 0.0
        out = torch.empty_like(x0)
        import ctypes

        lib = _hip.load()
        table = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
        _hip.upload_rows(table, 0, [_hip.IndexedRows.row_from(plan)])
        index = torch.zeros(1, dtype=torch.int32, device=dev)
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ops])
        desc = _hip.StepMaskC(mask.data_ptr(), _hip.BF16, 0, mask.numel() // BATCH, mask.numel() // BATCH)

        def rows_launch():
            _hip.check(lib.skr_step_launch_masked_indexed(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), None, out.numel(), table.data_ptr(), index.data_ptr(), 0,
                                                          _hip.current_stream_ptr(dev)), "skr_step_launch_masked_indexed")  # fmt: skip

        launches = {
            "masked": lambda: _hip.launch_step_masked(plan, ops, out, mask, mask.numel() // BATCH, mask.numel() // BATCH, None, out.numel(), dev),
            "rows": rows_launch,
            "plain": lambda: _hip.launch_step(plan, ops, out, None, None, out.numel(), dev),
        }
        for name, launch in launches.items():
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
            result[name + "_us"] = per
        result["operands"] = n
        result["masked_bytes"] = result["rows_bytes"] = out.numel() * 2 * (n + 1) + mask.numel() * 2
        result["plain_bytes"] = out.numel() * 2 * (n + 1)
        print("RESULT " + json.dumps(result), flush=True)
        return

    make = (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))) if sampler == "dpm2" else (lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled())))  # fmt: skip
    w = make()
    if form in ("a", "c"):
        w.set_inpaint(mask, orig, nz)
    inverse = 1 - mask

    if form == "c":
        from skrample_amd.graphs import capture_sampling_loop

        calls = [0]

        def model(x, t):  # the ring of fixed model outputs, in the order forms a and b read it (the capture freezes the sequence)
            calls[0] += 1
            return ring[(calls[0] - 1) & 3]

        loop = capture_sampling_loop(w, model, x0, steps, indexed=True, slots=1)
        for _ in range(2):
            loop(x0)
        torch.cuda.synchronize()
        event_us, wall_us = [], []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            loop(x0)
            e1.record()
            torch.cuda.synchronize()
            wall_us.append((time.perf_counter() - t0) * 1e6 / steps)
            event_us.append(e0.elapsed_time(e1) * 1e3 / steps)
        result.update(event_us=event_us, wall_us=wall_us, fast_hits=w._fast_hits)
        print("RESULT " + json.dumps(result), flush=True)
        return

    def loop():
        w.set_timesteps(steps)
        ts, tensor_ts = w.timesteps.tolist(), w.timesteps
        return ts, tensor_ts

    def run(ts, tensor_ts):
        x = x0
        if form == "a":
            for i, t in enumerate(ts):
                x = w.step(ring[i & 3], t, x, return_dict=False)[0]
        else:
            for i, t in enumerate(ts):
                prev = w.step(ring[i & 3], t, x, return_dict=False)[0]
                known = w.add_noise(orig, nz, tensor_ts[i + 1 : i + 2]) if i + 1 < len(ts) else orig
                x = mask * prev + inverse * known
        return x

    for _ in range(2):  # (two whole runs: the plain steps of form b are served by the replayed fast path from the second run on)
        run(*loop())
    torch.cuda.synchronize()
    event_us, wall_us = [], []
    for _ in range(repeats):
        ts, tensor_ts = loop()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        run(ts, tensor_ts)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_step.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200:
        ap.error("at least 5 repeats of at least 200 steps")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.steps)
        return 0
    lines = [f"masked steps: {BATCH} x {SHAPE} bf16 latents, (B, 1, H, W) bf16 mask, no network; {args.repeats} repeats of {args.steps} steps after two warm-up runs",
             "us per step: median (min - max) over the repeats; one child process per form and sampler"]  # fmt: skip
    failed = False
    for sampler in SAMPLERS:
        seen = {}
        for form in (*FORMS, "k"):
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--child", form, sampler],
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
            lines.append(f"  {form}  {what:26s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})   fast-path steps {seen[form]['fast_hits']}")
        (am, alo, ahi), (bm, blo, bhi) = summary(seen["a"]["wall_us"]), summary(seen["b"]["wall_us"])
        margin = (ahi - alo) + (bhi - blo)
        ok = bm - am > margin
        failed |= not ok
        lines.append(f"  wall-clock medians: b - a = {bm - am:.2f} us (b / a = {bm / am:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (a below b by more than the spreads)")
        (eam, _, _), (ebm, _, _) = summary(seen["a"]["event_us"]), summary(seen["b"]["event_us"])
        lines.append(f"  event-clock medians: b / a = {ebm / eam:.2f}")
        cm, clo, chi = summary(seen["c"]["wall_us"])
        margin = (ahi - alo) + (chi - clo)
        ok = am - cm > margin
        failed |= not ok
        lines.append(f"  wall-clock medians: a - c = {am - cm:.2f} us (a / c = {am / cm:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (c below a by more than the spreads)")
        k = seen["k"]
        (mm, mlo, mhi), (rm, _, _) = summary(k["masked_us"]), summary(k["rows_us"])
        lines.append(f"  k  row kernel median {rm:.2f} us against its kernarg twin's {mm:.2f} ({mlo:.2f} - {mhi:.2f}): {'inside' if mlo <= rm <= mhi else 'outside'} the twin's spread")
        for name in ("masked", "rows", "plain"):
            m, lo, hi = summary(k[name + "_us"])
            lines.append(f"  k  {name:6s} kernel, {k['operands']} operands   event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f}) per launch   {k[name + '_bytes'] / 1e6:7.1f} MB -> {k[name + '_bytes'] / (m * 1e-6) / PEAK * 100:5.1f} % of 8 TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
