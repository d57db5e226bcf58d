"""Cost of an eager DPM-2 step_guided loop under dynamic thresholding: the default route (guidance-only launch, statistic, step) against
set_thresholding(..., fuse_guidance=True) (guided statistic, guided step), bf16, batch 64.

  python tools/bench_guided_thresholding.py [--repeats 7] [--runs 20] [--out profiles/guided_thresholding.txt]

One child process per shape (the parent never opens the GPU).  Inside it the two forms of each pair ALTERNATE, repeat by repeat, on the
same device in the same state, so that a drift of the box falls on both:
  default / fused          step_guided() under set_thresholding(0.995, 1.5) without and with fuse_guidance=True
  statistic / g-statistic  skr_threshold_scale over a stored guided tensor / skr_guided_threshold_scale over uncond and cond, alone through
                           the C ABI (four kernels each; the workspace allocated once)
Per repeat, `runs` 20-step runs (wrapper forms) or 20 * runs calls (entry forms) are timed with HIP events around work that ends in a
synchronise, after a warm-up of 3 runs; reported per form: median and min - max over the repeats, us per step.  The verdict line says
whether the fused median lies below the default's by more than the two spreads (max - min) together."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"4x128x128": (64, 4, 128, 128), "3x64x64": (64, 3, 64, 64)}
PAIRS = (("default", "fused"), ("statistic", "g-statistic"))
STEPS, WARMUP, RATIO, MAX_VALUE, G = 20, 3, 0.995, 1.5, 7.5


def child(shape_name: str, repeats: int, runs: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.sampling import lazy
    from skrample_amd.sampling import structured as PT

    dev, shape, dtype = torch.device("cuda:0"), SHAPES[shape_name], torch.bfloat16
    g = torch.Generator().manual_seed(0)
    unconds, conds = ([torch.randn(shape, generator=g).to(dtype).to(dev) for _ in range(STEPS)] for _ in range(2))
    start = (torch.randn(shape, generator=g) * 14.6).to(dtype).to(dev)
    wrappers = {}
    for form in PAIRS[0]:
        wrappers[form] = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
        wrappers[form].set_thresholding(RATIO, MAX_VALUE, fuse_guidance=form == "fused")
    lib, stream, n, numel = _hip.load(), _hip.current_stream_ptr(dev), start[0].numel(), start.numel()
    scale = torch.empty(shape[0], dtype=torch.float32, device=dev)
    workspace = torch.empty(_hip.threshold_workspace(numel, n), dtype=torch.uint8, device=dev)
    code, stored = _hip.DTYPE_CODE[dtype], lazy.guide_only(lazy.Guidance(unconds[0], conds[0], G))

    def one_run(form):
        if form in wrappers:
            w, x = wrappers[form], start
            w.set_timesteps(STEPS)
            for i, t in enumerate(w.timesteps.tolist()):
                x = w.step_guided(unconds[i], conds[i], G, t, x, return_dict=False)[0]
            return x
        status = 0
        for _ in range(STEPS):
            if form == "statistic":
                status |= lib.skr_threshold_scale(start.data_ptr(), stored.data_ptr(), code, 0.07, -1.0, RATIO, MAX_VALUE, numel, n, scale.data_ptr(), workspace.data_ptr(), stream)
            else:
                status |= lib.skr_guided_threshold_scale(start.data_ptr(), unconds[0].data_ptr(), conds[0].data_ptr(), code, G, 0.07, -1.0, RATIO, MAX_VALUE, numel, n,
                                                         scale.data_ptr(), workspace.data_ptr(), stream)  # fmt: skip
        _hip.check(status, form)
        return scale

    event_us = {form: [] for pair in PAIRS for form in pair}
    for pair in PAIRS:
        for form in pair:
            for _ in range(WARMUP):
                one_run(form)
        torch.cuda.synchronize()
        for _ in range(repeats):
            for form in pair:  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(runs):
                    last = one_run(form)
                e1.record()
                torch.cuda.synchronize()
                event_us[form].append(e0.elapsed_time(e1) * 1e3 / (runs * STEPS))
                assert torch.isfinite(last.float()).all()
    same = torch.equal(one_run("default"), one_run("fused"))
    print("RESULT " + json.dumps({"shape": shape_name, "event_us": event_us, "same_bits": same, "device": torch.cuda.get_device_name(0)}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_thresholding.txt"))
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.repeats < 5 or args.runs < 5:
        ap.error("at least 5 repeats of at least 5 runs")
    if args.child:
        child(args.child, args.repeats, args.runs)
        return 0
    lines = [f"guided dynamic thresholding, DPM-2 step_guided, bf16, guidance {G}, ratio {RATIO}, sample_max_value {MAX_VALUE}; {args.repeats} repeats of {args.runs} runs of "
             f"{STEPS} steps after {WARMUP} warm-up runs, the two forms of a pair alternating in one process",
             "us per step (HIP events, host time of the loop included): median (min - max) over the repeats"]  # fmt: skip
    for shape_name, shape in SHAPES.items():
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--runs", str(args.runs), "--child", shape_name],
                             capture_output=True, text=True, timeout=540)  # fmt: skip
        found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
        if run.returncode != 0 or not found:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
            print(f"{shape_name} failed with exit status {run.returncode}: stopping", file=sys.stderr)
            return 1  # (nothing more is started on the device after a failure)
        seen = json.loads(found[-1][len("RESULT "):])
        lines.append(f"{shape[0]} x {shape_name}  ({seen['device']}); final samples of the two routes bit-equal: {seen['same_bits']}")
        for a, b in PAIRS:
            va, vb = seen["event_us"][a], seen["event_us"][b]
            for form, v in ((a, va), (b, vb)):
                lines.append(f"  {form:12s} {statistics.median(v):8.2f} ({min(v):8.2f} - {max(v):8.2f})")
            gain, spreads = statistics.median(va) - statistics.median(vb), (max(va) - min(va)) + (max(vb) - min(vb))
            lines.append(f"  {b} below {a} by {gain:.2f} us; the two spreads together {spreads:.2f} us: " + ("a gain beyond the spreads" if gain > spreads else "NO gain beyond the spreads"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
