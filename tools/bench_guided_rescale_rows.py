"""Cost of rescaled guidance with device-resident rows: a captured indexed rescaled loop against the indexed loop a user could capture
before it, against the `indexed=False` capture that freezes phi, and the row kernels against their kernarg twins.
256 x (4, 128, 128) bf16 latents, DPM-2, guidance scale 7.3, guidance_rescale 0.7.

  python tools/bench_guided_rescale_rows.py [--repeats 7] [--steps 200] [--out profiles/guided_rescale_rows.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  k  kernels alone     through the C ABI, 3 operands, storing p'.  The step: skr_step_launch_guided_rescaled (the yardstick, untouched),
                       skr_step_launch_guided_rescaled_indexed and ..._indexed_per_sample, taking turns within every repeat.  The
                       statistic: skr_guidance_rescale_factor, skr_guidance_rescale_factor_indexed and ..._indexed_per_sample, likewise.
                       Event clock per launch.
  g  rescaled loop     capture_sampling_loop(DPM-2, indexed=True, guidance_scale=7.3, guidance_rescale=0.7, rescaled=True) over an
                       elementwise two-output network: per step the network's two kernels, the statistics row launch (two kernels) and
                       ONE rescaled row step launch
  y  yardstick loop    what a user can capture with device-resident rows without the row forms: the same indexed loop whose model returns
                       diffusers' lines -- u + g * (c - u), the two stds, the division, resc, the blend: nine torch kernels -- then the
                       plain indexed step launch
  f  frozen loop       the indexed=False rescaled capture: the same launches with scale and phi frozen into the graph
Loops are LOOP_STEPS long and replayed steps / LOOP_STEPS times per repeat, timed with HIP events around the replays (graph.replay()
alone: no copy in, no clone out); reported per form: median and min - max over the repeats, us per step.

Expectations, stated before the run.  Tensor passes per step behind the network: g moves 8 (the statistic reads uncond and cond; the step
reads uncond, cond, the sample and the previous prediction and writes the sample and the prediction), y moves 23 (torch's nine kernels
read and write whole tensors, then the step's four).  No ratio is fixed in advance: the statistics launch is bound by fp64 issue, not by
bytes.  (a) JUDGED: g's median is below y's by more than the two forms' min - max spreads put together.  (b) reported: g against f, which
profiles/guided_rescale.txt has at 62.96 us on the parent commit -- g should sit on it, or above it by a dependent scalar load or two per
launch (an index entry, then a row: three launches a step read them).  (c) reported: the row step kernels equal the kernarg twin within
the spreads or sit above it by those scalar loads; the indexed statistic likewise."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, WARMUP, SCALE, PHI, LOOP_STEPS = 256, (4, 128, 128), 20, 7.3, 0.7, 50
LOOPS = {"g": "rescaled loop (row launches)", "y": "torch lines in the model + step", "f": "indexed=False rescaled capture"}
STEP_KERNELS = (("kernarg", "skr_step_launch_guided_rescaled"), ("indexed", "skr_step_launch_guided_rescaled_indexed"),
                ("per_sample", "skr_step_launch_guided_rescaled_indexed_per_sample"))  # fmt: skip
STAT_KERNELS = (("stat_kernarg", "skr_guidance_rescale_factor"), ("stat_indexed", "skr_guidance_rescale_factor_indexed"),
                ("stat_per_sample", "skr_guidance_rescale_factor_indexed_per_sample"))  # fmt: skip


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
        sample_numel = SHAPE[0] * SHAPE[1] * SHAPE[2]
        numel, n = BATCH * sample_numel, 3
        stream = _hip.current_stream_ptr(dev)
        ops, cond = [fresh() for _ in range(n)], fresh()
        out, guided = torch.empty_like(cond), torch.empty_like(cond)
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = n
        plan.dtype_a = plan.out0_dtype = _hip.BF16
        plan.dtype_b, plan.out1_dtype = _hip.F32, _hip.NONE
        plan.sample_numel = sample_numel
        row = _hip.StepRowC()
        for k in range(n):
            plan.coef0[k] = row.coef0[k] = 0.5 - 0.1 * k
        row.convert_k[0], row.convert_k[1] = SCALE, PHI
        table = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
        _hip.upload_rows(table, 0, [row])
        index, sample_index = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(BATCH, dtype=torch.int32, device=dev)
        factor = torch.zeros(BATCH, dtype=torch.bfloat16, device=dev)
        partials = torch.zeros(_hip.guidance_partials(numel, sample_numel), dtype=torch.float64, device=dev)
        arr = _hip._operand_array(ops)
        guide = _hip.StepGuidanceC(cond.data_ptr(), guided.data_ptr(), SCALE, 1, 0)
        rescale = _hip.StepRescaleC(factor.data_ptr(), PHI, sample_numel, 0)
        head = (ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(rescale), None, numel)
        stat_head = (ops[1].data_ptr(), cond.data_ptr(), _hip.BF16)
        stat_tail = (factor.data_ptr(), None, partials.data_ptr(), stream)

        def run(status):
            if status != 0:
                raise SystemExit(f"launch refused with status {status}")

        stats = {
            "stat_kernarg": lambda: run(lib.skr_guidance_rescale_factor(*stat_head, SCALE, numel, sample_numel, *stat_tail)),
            "stat_indexed": lambda: run(lib.skr_guidance_rescale_factor_indexed(*stat_head, numel, sample_numel, table.data_ptr(), index.data_ptr(), 0, *stat_tail)),
            "stat_per_sample": lambda: run(lib.skr_guidance_rescale_factor_indexed_per_sample(*stat_head, numel, sample_numel, table.data_ptr(), sample_index.data_ptr(), 0, *stat_tail)),
        }
        steps_of = {
            "kernarg": lambda: run(lib.skr_step_launch_guided_rescaled(*head, stream)),
            "indexed": lambda: run(lib.skr_step_launch_guided_rescaled_indexed(*head, table.data_ptr(), index.data_ptr(), 0, stream)),
            "per_sample": lambda: run(lib.skr_step_launch_guided_rescaled_indexed_per_sample(*head, table.data_ptr(), sample_index.data_ptr(), 0, stream)),
        }
        wants = {}
        for name, launch in stats.items():  # (the three forms write the same bits: checked at the size that is timed)
            factor.zero_()
            launch()
            wants[name] = (factor.clone(),)
        for name, launch in steps_of.items():
            out.zero_(), guided.zero_()
            launch()
            wants[name] = (out.clone(), guided.clone())
        same = lambda a, b: all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(wants[a], wants[b]))  # noqa: E731
        result["same_bits"] = all(same(name, "kernarg") for name in ("indexed", "per_sample")) and all(same(name, "stat_kernarg") for name in ("stat_indexed", "stat_per_sample"))
        for group in (steps_of, stats):
            for launch in group.values():
                timed_once(launch, WARMUP)
            per = {name: [] for name in group}
            for _ in range(repeats):
                for name, launch in group.items():  # the forms take turns within a repeat
                    per[name].append(timed_once(launch, steps) / steps)
            for name in group:
                result[f"{name}_us"] = per[name]
        print("RESULT " + json.dumps(result), flush=True)
        return

    def net(x, t):  # elementwise, two outputs: the halves of a doubled-batch network output
        return x * 0.5, x * 0.25

    def lines(x, t):  # what a user writes inside the captured model without the row forms: diffusers' lines
        u, c = net(x, t)
        p = u + SCALE * (c - u)
        std_text = c.std(dim=list(range(1, c.ndim)), keepdim=True)
        std_cfg = p.std(dim=list(range(1, p.ndim)), keepdim=True)
        resc = p * (std_text / std_cfg)
        return PHI * resc + (1 - PHI) * p

    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    x0 = fresh()
    if form == "g":
        loop = capture_sampling_loop(w, net, x0, LOOP_STEPS, indexed=True, guidance_scale=SCALE, guidance_rescale=PHI, rescaled=True)
    elif form == "y":
        loop = capture_sampling_loop(w, lines, x0, LOOP_STEPS, indexed=True)
    else:
        loop = capture_sampling_loop(w, net, x0, LOOP_STEPS, guidance_scale=SCALE, guidance_rescale=PHI)
    result["launches_per_loop"] = loop.rows.length if loop.rows is not None else LOOP_STEPS
    result["checksum"] = float(loop(x0).float().abs().mean())  # (the forms compute the same loop: printed beside the times)
    replays = steps // LOOP_STEPS
    timed_once(loop.graph.replay, 2)
    result["event_us"] = [timed_once(loop.graph.replay, replays) / (replays * LOOP_STEPS) for _ in range(repeats)]
    print("RESULT " + json.dumps(result), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_rescale_rows.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.steps < 200 or args.steps % LOOP_STEPS != 0:
        ap.error(f"at least 5 repeats of at least 200 steps, a multiple of {LOOP_STEPS}")
    if args.child:
        child(args.child, args.repeats, args.steps)
        return 0

    def spawn(form):
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--steps", str(args.steps), "--child", form],
                             capture_output=True, text=True, timeout=300)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return None  # (nothing more is started on the device after a failure)
        return json.loads(found[-1][len("RESULT "):])

    seen = {}
    for form in LOOPS:
        seen[form] = spawn(form)
        if seen[form] is None:
            return 1
    device = seen["g"]["device"]
    lines = [f"rescaled guidance with device-resident rows: {BATCH} x {SHAPE} bf16 latents, DPM-2, guidance scale {SCALE}, guidance_rescale {PHI}; "
             f"{args.repeats} repeats of {args.steps} steps  ({device})",
             "us: median (min - max) over the repeats; one child process per form",
             f"(a) captured DPM-2 loops of {LOOP_STEPS} steps over an elementwise two-output network, replayed {args.steps // LOOP_STEPS} times per repeat; us per step"]  # fmt: skip
    for form, what in LOOPS.items():
        m, lo, hi = summary(seen[form]["event_us"])
        lines.append(f"  {form}  {what:34s} event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f})   step launches per loop {seen[form]['launches_per_loop']}   mean |x| {seen[form]['checksum']:.6f}")
    (gm, glo, ghi), (ym, ylo, yhi), (fm, flo, fhi) = (summary(seen[form]["event_us"]) for form in "gyf")
    margin = (ghi - glo) + (yhi - ylo)
    ok = ym - gm > margin
    lines.append(f"  JUDGED  medians: y - g = {ym - gm:.2f} us per step (y / g = {ym / gm:.2f}), the two spreads together {margin:.2f} us: {'PASS' if ok else 'FAIL'} (g below y by more than the spreads)")
    margin = (ghi - glo) + (fhi - flo)
    verdict = "equal within the two spreads together" if abs(gm - fm) <= margin else ("above the frozen capture" if gm > fm else "below the frozen capture")
    lines.append(f"  (b) medians: g - f = {gm - fm:+.2f} us per step, the two spreads together {margin:.2f} us: {verdict} (reported, not judged)")
    k = spawn("k")
    if k is None:
        return 1
    lines.append("(c) kernels alone, through the C ABI, 3 operands, storing p'; the three forms of a launch take turns within every repeat")
    for group in (STEP_KERNELS, STAT_KERNELS):
        base = group[0][0]
        (km, klo, khi) = summary(k[f"{base}_us"])
        for name, what in group:
            m, lo, hi = summary(k[f"{name}_us"])
            lines.append(f"  k  {what:52s} event clock {m:8.2f} ({lo:8.2f} - {hi:8.2f}) per launch")
        for name, _ in group[1:]:
            m, lo, hi = summary(k[f"{name}_us"])
            margin = (hi - lo) + (khi - klo)
            verdict = "equal within the two spreads together" if abs(m - km) <= margin else ("above the kernarg twin" if m > km else "below the kernarg twin")
            lines.append(f"  k  {name} - {base} = {m - km:+.2f} us, the two spreads together {margin:.2f} us: {verdict} (reported, not judged)")
    lines.append(f"  k  the row forms wrote the bits of their kernarg twins at this size: {k['same_bits']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
