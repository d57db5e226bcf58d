"""Cost of a scheduler step on channels-last latents: run in place (skr_step_launch_channels_last) against the copies made before.
256 x (4, 128, 128) bf16 through SkrampleWrapperScheduler.step, DPM-2 eta = 1 (the headline step: Philox noise in registers) and eta = 0.

  python tools/bench_channels_last.py [--repeats 5] [--steps 200] [--out profiles/channels_last.txt] [--operands 4] [--channels 4]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  channels-last, in place    sample and model_output in torch.channels_last: one launch on the caller's tensors, channels-last result
  b  channels-last, copied      the same calls with lazy.channels_last = False: every non-contiguous operand is copied first and the result
                                is contiguous -- what the engine did before it knew the layout, and the yardstick
  c  contiguous                 contiguous sample and model_output (the path the engine was tuned on)
  k  kernels alone              skr_step_launch_channels_last (step_kernel_cl1<bf16, 4, 4>) on channels-last operands beside skr_step_launch on
                                contiguous ones (step_kernel_k1<bf16, 4, noise>, paced as shipped and with "pace" 0 -- the form the new kernel was
                                derived from), 4 operands + Philox, rounds interleaved in one process: event clock per launch and the fraction
                                of 8 TB/s the algorithmic bytes (4 loads + 1 store) come to; and the general kernel ("one_trip" 0) on the same.
                                --operands K --channels C time step_kernel_cl1<bf16, K, C> instead, on 256 x (C, 128, 512 / C)
A run is `steps` steps of one schedule; the result of a step is the next step's sample, the model outputs rotate through six distinct
tensors in the form's layout (form a and b: a channels-last network hands back channels-last; distinct buffers, as a network's are, let
the wrapper's history alias them instead of taking snapshots).  Three warm-up runs (from the second on the replayed
fast path serves the steps where the form has one), then per repeat one run timed with HIP events (first enqueue to last kernel) and with the wall
clock (first call to the end of a device synchronisation); reported per form: median and min - max over the repeats, us per step.
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
SHAPE, WARMUP_RUNS, NBUF = (256, 4, 128, 128), 3, 6
SAMPLERS = {"dpm2_sde": "DPM-2, eta = 1", "dpm2": "DPM-2, eta = 0"}
FORMS = {"a": "channels-last, in place", "b": "channels-last, copied", "c": "contiguous"}
PEAK = 8.0e12  # bytes per second


def child(form: str, sampler: str, repeats: int, steps: int, operands: int = 4, channels: int = 4) -> None:
    import ctypes

    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.sampling import lazy
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    shape = SHAPE if form != "k" else (SHAPE[0], channels, SHAPE[2], SHAPE[3] * SHAPE[1] // channels)  # (as many elements whatever the channel count)
    fresh = lambda: torch.randn(shape, generator=g).bfloat16().to(dev)  # noqa: E731
    result = {"form": form, "sampler": sampler, "device": torch.cuda.get_device_name(0)}
    lib = _hip.load()

    if form == "k":
        n = operands
        ops = [fresh() for _ in range(n)]
        ops_cl = [t.contiguous(memory_format=torch.channels_last) for t in ops]
        out, out_cl = torch.empty_like(ops[0]), torch.empty_like(ops_cl[0])
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = n
        plan.dtype_a = plan.out0_dtype = _hip.BF16
        plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
        plan.sample_numel, plan.noise_mode, plan.zeta0, plan.stream0 = out[0].numel(), 1, 0.3, 256
        for k in range(n):
            plan.coef0[k] = 1.0 / n
        seeds = torch.arange(1, SHAPE[0] + 1, dtype=torch.int64, device=dev)
        arr, arr_cl = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in group]) for group in (ops, ops_cl))
        layout = _hip.StepLayoutC(shape[1], shape[2] * shape[3])
        stream = _hip.current_stream_ptr(dev)

        def contiguous():
            _hip.check(lib.skr_step_launch(ctypes.byref(plan), arr, out.data_ptr(), None, seeds.data_ptr(), out.numel(), stream), "skr_step_launch")

        def channels_last():
            _hip.check(lib.skr_step_launch_channels_last(ctypes.byref(plan), arr_cl, out_cl.data_ptr(), None, seeds.data_ptr(), ctypes.byref(layout), out.numel(), stream), "skr_step_launch_channels_last")

        cases = (("k1_paced", contiguous, ()), ("k1_unpaced", contiguous, ((b"pace", 0),)), ("cl1", channels_last, ()), ("cl_general", channels_last, ((b"one_trip", 0),)))
        for name, _, _ in cases:
            result[name + "_us"] = []
        for rep in range(repeats + 1):  # (round 0 warms every form up)
            for name, launch, switches in cases:
                for key, value in switches:
                    lib.skr_set_tuning(key, value)
                count = steps if name != "cl_general" else max(steps // 10, 10)
                launch()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(count):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                lib.skr_set_tuning(b"reset", 0)
                if rep:
                    result[name + "_us"].append(e0.elapsed_time(e1) * 1e3 / count)
        assert torch.equal(out_cl, out)  # the same bits, viewed logically
        result["operands"], result["channels"] = n, channels
        result["bytes"] = out.numel() * 2 * (n + 1)
        print("RESULT " + json.dumps(result), flush=True)
        return

    lazy.channels_last = form != "b"
    place = (lambda t: t) if form == "c" else (lambda t: t.contiguous(memory_format=torch.channels_last))
    eta = 1.0 if sampler == "dpm2_sde" else 0.0
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=eta), PS.Karras(PS.Scaled()))
    x0, model_outputs = place(fresh()), [place(fresh() * 0.1) for _ in range(NBUF)]
    seeds = list(range(1, SHAPE[0] + 1))

    def run():
        w.set_timesteps(steps)
        x = x0
        for i, t in enumerate(w.timesteps.tolist()):
            x = w.step(model_outputs[i % NBUF], t, x, generator=seeds, return_dict=False)[0]
        return x

    for _ in range(WARMUP_RUNS):
        last = run()
    torch.cuda.synchronize()
    event_us, wall_us = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        last = run()
        e1.record()
        torch.cuda.synchronize()
        wall_us.append((time.perf_counter() - t0) * 1e6 / steps)
        event_us.append(e0.elapsed_time(e1) * 1e3 / steps)
    want_layout = torch.contiguous_format if form != "a" else torch.channels_last
    assert last.is_contiguous(memory_format=want_layout), (form, last.stride())
    result.update(event_us=event_us, wall_us=wall_us, fast_hits=w._fast_hits, checksum=float(last.contiguous().float().abs().mean()))  # (one reduction order whatever the layout)
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channels_last.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SAMPLER"))
    ap.add_argument("--tree", default=None, help="time the package of this source tree instead (tools/bench_channels_last_shared.py: a parent commit beside this one)")
    ap.add_argument("--operands", type=int, default=4, choices=range(1, 9), help="form k: operands of the launch")
    ap.add_argument("--channels", type=int, default=4, choices=(4, 8, 16), help="form k: channels of the latents")
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200:
        ap.error("at least 5 repeats of at least 200 steps")
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.steps, args.operands, args.channels)
        return 0
    lines = [f"scheduler steps on channels-last latents: {SHAPE[0]} x {SHAPE[1:]} bf16 through SkrampleWrapperScheduler.step; "
             f"{args.repeats} repeats of {args.steps} steps after {WARMUP_RUNS} warm-up runs",
             "us per step: median (min - max) over the repeats; one child process per form and sampler"]  # fmt: skip
    failed = False

    def spawn(form, sampler):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--operands", str(args.operands),
                              "--channels", str(args.channels), "--child", form, sampler],
                             capture_output=True, text=True, timeout=600)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} / {sampler} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        return json.loads(found[-1][len("RESULT "):])

    for sampler, what in SAMPLERS.items():
        seen = {}
        for form in FORMS:
            seen[form] = spawn(form, sampler)
            if seen[form] is None:
                return 1
        lines.append(f"{sampler}  ({what}; {seen['a']['device']})")
        for form, name in FORMS.items():
            (em, elo, ehi), (wm, wlo, whi) = summary(seen[form]["event_us"]), summary(seen[form]["wall_us"])
            lines.append(f"  {form}  {name:26s} event clock {em:8.2f} ({elo:8.2f} - {ehi:8.2f})   wall clock {wm:8.2f} ({wlo:8.2f} - {whi:8.2f})   fast-path steps {seen[form]['fast_hits']}")
        if len({seen[form]["checksum"] for form in FORMS}) != 1:
            lines.append("  the three forms DISAGREE on the last result: " + ", ".join(f"{form} {seen[form]['checksum']!r}" for form in FORMS))
            failed = True
        (am, alo, ahi), (bm, blo, bhi) = summary(seen["a"]["wall_us"]), summary(seen["b"]["wall_us"])
        margin = (ahi - alo) + (bhi - blo)
        ok = bm - am > margin
        failed |= not ok
        lines.append(f"  wall-clock medians: b - a = {bm - am:.2f} us (b / a = {bm / am:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (a below b by more than the spreads)")
        (eam, _, _), (ebm, _, _), (ecm, _, _) = summary(seen["a"]["event_us"]), summary(seen["b"]["event_us"]), summary(seen["c"]["event_us"])
        lines.append(f"  event-clock medians: b / a = {ebm / eam:.2f}, a / c = {eam / ecm:.3f}")
    k = spawn("k", "dpm2_sde")
    if k is None:
        return 1
    lines.append(f"kernels alone  ({k['operands']} bf16 operands + Philox, {k['bytes'] / 1e6:.1f} MB of algorithmic bytes per launch; rounds interleaved in one process)")
    n, c = k["operands"], k["channels"]
    for name, kernel in (("k1_paced", f"step_kernel_k1<bf16, {n}, noise, paced>   contiguous"), ("k1_unpaced", f"step_kernel_k1<bf16, {n}, noise, unpaced> contiguous"),
                         ("cl1", f"step_kernel_cl1<bf16, {n}, {c}>".ljust(40) + "channels-last"), ("cl_general", "step_kernel_cl<float> (general)         channels-last")):  # fmt: skip
        m, lo, hi = summary(k[name + "_us"])
        lines.append(f"  k  {kernel:56s} event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f}) per launch   {k['bytes'] / (m * 1e-6) / PEAK * 100:5.1f} % of 8 TB/s")
    (cm, clo, chi), (um, ulo, uhi) = summary(k["cl1_us"]), summary(k["k1_unpaced_us"])
    inside = abs(cm - um) <= (uhi - ulo)
    lines.append(f"  cl1 - k1 unpaced = {cm - um:+.2f} us; the twin's run-to-run spread {uhi - ulo:.2f} us: {'within' if inside else 'OUTSIDE'} the spread")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
