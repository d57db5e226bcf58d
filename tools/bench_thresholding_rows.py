"""Cost of a DPM-2 step under dynamic thresholding in captured loops against the eager loop, and of the statistics row launch against the
direct statistic; bf16, 64 x (4, 128, 128).

  python tools/bench_thresholding_rows.py [--repeats 7] [--runs 20] [--out profiles/thresholding_rows.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  eager            step() under set_thresholding(0.995, 1.5), launch by launch (tools/bench_thresholding.py's `wrapper`)
  frozen           capture_sampling_loop(..., thresholded=True): the eager launches in one graph
  indexed          ... indexed=True: the statistics row launch and the row step, one row for the batch
  per_sample       ... per_sample=True: one row per sample
  statistic        skr_threshold_scale alone through the C ABI (its four kernels; the workspace allocated once)
  statistic_rows   skr_threshold_scale_indexed alone through the C ABI, the same values in a row
  statistic_each   skr_threshold_scale_indexed_per_sample alone, every sample on that row
The network of the loop forms is one elementwise launch (x * 0.5), so a step is that launch, the statistic and the thresholded step.  Per
repeat, `runs` 20-step loops (or 20 * runs entry calls) are timed with HIP events after a warm-up of 3; reported per form: median and min -
max over the repeats, us per step."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPE = (64, 4, 128, 128)
FORMS = {"eager": "eager thresholded loop", "frozen": "captured, indexed=False", "indexed": "captured, indexed=True", "per_sample": "captured, per_sample=True",
         "statistic": "skr_threshold_scale", "statistic_rows": "skr_threshold_scale_indexed", "statistic_each": "skr_threshold_scale_indexed_per_sample"}  # fmt: skip
STEPS, WARMUP, RATIO, MAX_VALUE = 20, 3, 0.995, 1.5


def child(form: str, repeats: int, runs: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.graphs import capture_sampling_loop
    from skrample_amd.sampling import structured as PT

    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    g = torch.Generator().manual_seed(0)
    start = (torch.randn(SHAPE, generator=g) * 14.6).to(dtype).to(dev)
    net = lambda x, t: x * 0.5  # noqa: E731
    if not form.startswith("statistic"):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
        w.set_thresholding(RATIO, MAX_VALUE)
        if form == "eager":

            def one_run():
                w.set_timesteps(STEPS)
                x = start
                for t in w.timesteps.tolist():
                    x = w.step(net(x, t), t, x, return_dict=False)[0]
                return x
        else:
            loop = capture_sampling_loop(w, net, start, STEPS, indexed=form != "frozen", per_sample=form == "per_sample", thresholded=True)
            one_run = lambda: loop(start)  # noqa: E731
    else:
        lib, stream, n, numel = _hip.load(), _hip.current_stream_ptr(dev), start[0].numel(), start.numel()
        other = torch.randn(SHAPE, generator=g).to(dtype).to(dev)
        scale = torch.empty(SHAPE[0], dtype=torch.float32, device=dev)
        workspace = torch.empty(_hip.threshold_workspace(numel, n), dtype=torch.uint8, device=dev)
        code = _hip.DTYPE_CODE[dtype]
        row = _hip.StepRowC()
        row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3] = 0.07, -1.0, RATIO, MAX_VALUE
        rows = torch.zeros(ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=dev)
        _hip.upload_rows(rows, 0, [row])
        index = torch.zeros(SHAPE[0], dtype=torch.int32, device=dev)
        entry = lib.skr_threshold_scale_indexed_per_sample if form == "statistic_each" else lib.skr_threshold_scale_indexed

        def one_run():
            status = 0
            for _ in range(STEPS):
                if form == "statistic":
                    status |= lib.skr_threshold_scale(start.data_ptr(), other.data_ptr(), code, 0.07, -1.0, RATIO, MAX_VALUE, numel, n, scale.data_ptr(), workspace.data_ptr(), stream)
                else:
                    status |= entry(start.data_ptr(), other.data_ptr(), code, numel, n, rows.data_ptr(), index.data_ptr(), 0, scale.data_ptr(), workspace.data_ptr(), stream)
            _hip.check(status, form)
            return scale

    for _ in range(WARMUP):
        one_run()
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(runs):
            last = one_run()
        e1.record()
        torch.cuda.synchronize()
        event_us.append(e0.elapsed_time(e1) * 1e3 / (runs * STEPS))
    assert torch.isfinite(last.float()).all()
    print("RESULT " + json.dumps({"form": form, "event_us": event_us, "device": torch.cuda.get_device_name(0)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thresholding_rows.txt"))
    ap.add_argument("--child", metavar="FORM")
    args = ap.parse_args()
    if args.repeats < 5 or args.runs < 5:
        ap.error("at least 5 repeats of at least 5 runs")
    if args.child:
        child(args.child, args.repeats, args.runs)
        return 0
    lines = [f"dynamic thresholding in captured loops, DPM-2, bf16, {SHAPE[0]} x {SHAPE[1:]}, ratio {RATIO}, sample_max_value {MAX_VALUE}; {args.repeats} repeats of {args.runs} runs of "
             f"{STEPS} steps after {WARMUP} warm-up runs", "us per step (HIP events, host time included): median (min - max) over the repeats; one child process per form"]  # fmt: skip
    for form, what in FORMS.items():
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--runs", str(args.runs), "--child", form], capture_output=True, text=True, timeout=300)
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return 1  # (nothing more is started on the device after a failure)
        v = json.loads(found[-1][len("RESULT "):])
        if len(lines) == 2:
            lines.append(f"({v['device']})")
        lines.append(f"  {form:15s} {what:40s} {statistics.median(v['event_us']):8.2f} ({min(v['event_us']):8.2f} - {max(v['event_us']):8.2f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
