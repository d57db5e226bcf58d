"""Cost of a DPM-2 step under dynamic thresholding against torch's own lines in front of the unchanged step, bf16, batch 64.

  python tools/bench_thresholding.py [--repeats 7] [--runs 20] [--out profiles/thresholding.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU), per shape:
  torch      diffusers' _threshold_sample written out -- float(), abs, quantile, clamp, clamp / div, cast -- on x0 = a x + b o, then step()
             of a DataModel wrapper: the yardstick, code this change does not touch
  wrapper    step() under set_thresholding(0.995, 1.5): skr_threshold_scale, then skr_thresholded_step_launch
  statistic  skr_threshold_scale alone through the C ABI (its four kernels together; the workspace allocated once)
  step       skr_thresholded_step_launch alone through the C ABI (3 operands, no draw), on the scale the statistic wrote
Per repeat, `runs` 20-step runs (wrapper forms) or 20 * runs calls (entry forms) are timed with HIP events after a warm-up of 3 runs;
reported per form: median and min - max over the repeats, us per step.  The wrapper child also records how far s moves when the rank
is formed in fp32, as torch forms it, instead of double (first step of the run, in fp32 units in the last place of s)."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"4x128x128": (64, 4, 128, 128), "3x64x64": (64, 3, 64, 64)}
FORMS = {"torch": "torch's lines + DataModel step()", "wrapper": "step() under set_thresholding", "statistic": "skr_threshold_scale alone", "step": "skr_thresholded_step_launch alone"}
STEPS, WARMUP, RATIO, MAX_VALUE = 20, 3, 0.995, 1.5


def child(form: str, shape_name: str, repeats: int, runs: int) -> None:
    import numpy as np
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.sampling import models
    from skrample_amd.sampling import structured as PT

    dev, shape, dtype = torch.device("cuda:0"), SHAPES[shape_name], torch.bfloat16
    g = torch.Generator().manual_seed(0)
    outputs = [torch.randn(shape, generator=g).to(dtype).to(dev) for _ in range(STEPS)]
    start = (torch.randn(shape, generator=g) * 14.6).to(dtype).to(dev)
    extra = {}
    if form in ("torch", "wrapper"):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()), *([models.DataModel()] if form == "torch" else []))
        if form == "wrapper":
            w.set_thresholding(RATIO, MAX_VALUE)
        noise_model = models.NoiseModel()

        def one_run():
            w.set_timesteps(STEPS)
            x = start
            for i, t in enumerate(w.timesteps.tolist()):
                if form == "torch":
                    a, b = noise_model.x_weights(PT._ipoint(w.schedule, i / STEPS))
                    x0 = a * x + b * outputs[i]
                    flat = x0.float().reshape(shape[0], -1)
                    s = torch.quantile(flat.abs(), RATIO, dim=1).clamp(min=1, max=MAX_VALUE).unsqueeze(1)
                    p = (torch.clamp(flat, -s, s) / s).reshape(shape).to(dtype)
                    x = w.step(p, t, x, return_dict=False)[0]
                else:
                    x = w.step(outputs[i], t, x, return_dict=False)[0]
            return x

        calls = runs
        if form == "wrapper":  # the rank in fp32 (torch's) against the rank in double, in s
            a, b = noise_model.x_weights(PT._ipoint(PS.Karras(PS.Scaled()), 0.0))
            ours = torch.empty(shape[0], dtype=torch.float32, device=dev)
            n = start[0].numel()
            _hip.launch_threshold_scale(start, outputs[0], a, b, RATIO, 1e30, n, ours)
            x0 = np.float32(a) * start.float().cpu().numpy() + np.float32(b) * outputs[0].float().cpu().numpy()
            theirs = torch.quantile(torch.from_numpy(np.abs(x0)).reshape(shape[0], -1), RATIO, dim=1).clamp(min=1)
            units = (ours.cpu().view(torch.int32).long() - theirs.view(torch.int32).long()).abs()
            extra = {"rank_fp32_units_max": int(units.max()), "rank_fp32_samples_differing": int((units != 0).sum())}
    else:
        lib, stream, n, numel = _hip.load(), _hip.current_stream_ptr(dev), start[0].numel(), start.numel()
        scale = torch.empty(shape[0], dtype=torch.float32, device=dev)
        workspace = torch.empty(_hip.threshold_workspace(numel, n), dtype=torch.uint8, device=dev)
        code = _hip.DTYPE_CODE[dtype]
        _hip.launch_threshold_scale(start, outputs[0], 0.07, -1.0, RATIO, MAX_VALUE, n, scale)
        out, p = torch.empty_like(start), torch.empty_like(start)
        plan = _hip.StepPlanC()
        plan.n_terms = plan.n_group_a = 3
        plan.dtype_a = plan.dtype_b = plan.out0_dtype = code
        plan.out1_dtype = _hip.NONE
        plan.coef0[0], plan.coef0[1], plan.coef0[2] = 0.8, 0.3, -0.1
        operands = _hip._operand_array([start, outputs[0], outputs[1]])
        thr = _hip.StepThresholdC(scale.data_ptr(), p.data_ptr(), 0.07, -1.0, n, 1, 0, 0)

        def one_run():
            status = 0
            for _ in range(STEPS):
                if form == "statistic":
                    status |= lib.skr_threshold_scale(start.data_ptr(), outputs[0].data_ptr(), code, 0.07, -1.0, RATIO, MAX_VALUE, numel, n, scale.data_ptr(), workspace.data_ptr(), stream)
                else:
                    status |= lib.skr_thresholded_step_launch(plan, operands, out.data_ptr(), thr, None, numel, stream)
            _hip.check(status, form)
            return out

        calls = runs
    for _ in range(WARMUP):
        one_run()
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            last = one_run()
        e1.record()
        torch.cuda.synchronize()
        event_us.append(e0.elapsed_time(e1) * 1e3 / (calls * STEPS))
    assert torch.isfinite(last.float()).all()
    print("RESULT " + json.dumps({"form": form, "shape": shape_name, "event_us": event_us, "device": torch.cuda.get_device_name(0), **extra}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thresholding.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "SHAPE"))
    args = ap.parse_args()
    if args.repeats < 5 or args.runs < 5:
        ap.error("at least 5 repeats of at least 5 runs")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.runs)
        return 0
    lines = [f"dynamic thresholding, DPM-2, bf16, ratio {RATIO}, sample_max_value {MAX_VALUE}; {args.repeats} repeats of {args.runs} runs of {STEPS} steps after {WARMUP} warm-up runs",
             "us per step (HIP events, host time of the loop included): median (min - max) over the repeats; one child process per form and shape"]  # fmt: skip
    for shape_name, shape in SHAPES.items():
        seen = {}
        for form in FORMS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--runs", str(args.runs), "--child", form, shape_name],
                                 capture_output=True, text=True, timeout=600)  # fmt: skip
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"{shape_name} / form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[form] = json.loads(found[-1][len("RESULT "):])
        lines.append(f"{shape[0]} x {shape_name}  ({seen['torch']['device']})")
        for form, what in FORMS.items():
            v = seen[form]["event_us"]
            lines.append(f"  {form:10s} {what:36s} {statistics.median(v):8.2f} ({min(v):8.2f} - {max(v):8.2f})")
        lines.append(f"  wrapper / torch = {statistics.median(seen['wrapper']['event_us']) / statistics.median(seen['torch']['event_us']):.2f}")
        lines.append(f"  s with torch's fp32 rank against the double rank, first step: {seen['wrapper']['rank_fp32_samples_differing']} of {shape[0]} samples differ, "
                     f"by at most {seen['wrapper']['rank_fp32_units_max']} fp32 units in the last place")  # fmt: skip
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
