"""Cost of the masked backward launch beside the plain one: skr_step_masked_backward_launch against skr_step_backward_launch.
256 x (4, 128, 128) bf16, a (B, 1, H, W) bf16 mask, five gradients of one incoming gradient -- the backward of a DPM-2 in-painting step
(sample, model output, one history output, original, noise).  By bytes the masked launch moves (1 + 0.25 + 5) / (1 + 5) = 1.04 times
the plain one's traffic.

  python tools/bench_masked_backward.py [--repeats 7] [--launches 200] [--out profiles/masked_backward.txt]

One process; the two launches alternate, window by window: per repeat, `launches` back-to-back launches of each are timed with HIP
events.  Reported: median and min - max over the repeats in us per launch, the ratio of the medians beside the byte ratio, and whether
the excess over the byte ratio is larger than the run-to-run spread seen (the two relative spreads put together).  Nothing is judged:
the exit status is 0 whenever the launches ran."""

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, GRADS, WARMUP = 256, (4, 128, 128), 5, 20
PEAK = 8.0e12  # bytes per second


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_backward.txt"))
    args = ap.parse_args()
    if args.repeats < 5 or args.launches < 100:
        ap.error("at least 5 repeats of at least 100 launches")
    import torch

    from skrample_amd import _hip

    dev = torch.device("cuda:0")
    lib = _hip.load()
    shape = (BATCH, *SHAPE)
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(shape, generator=gen).bfloat16().to(dev)
    mask = (torch.rand((BATCH, 1, *SHAPE[1:]), generator=gen) < 0.5).bfloat16().to(dev)
    grads = [torch.empty_like(g) for _ in range(GRADS)]
    plan = _hip.StepGradPlanC()
    plan.n_grads = plan.n_group_a = GRADS
    plan.dtype_a = plan.dtype_b = plan.g0_dtype = _hip.BF16
    plan.g1_dtype = _hip.NONE
    for k in range(GRADS):  # the step form holds the first three operands, the known form the last two
        plan.a[k], plan.b[k] = (0.5, 0.0) if k < 3 else (0.0, 0.5)
    arr = (ctypes.c_void_p * GRADS)(*[t.data_ptr() for t in grads])
    mask_numel = mask.numel() // BATCH
    desc = _hip.StepMaskC(mask.data_ptr(), _hip.BF16, 0, mask_numel, mask_numel)
    stream = _hip.current_stream_ptr(dev)
    numel, sample_numel = g.numel(), g[0].numel()
    launches = {
        "masked": lambda: _hip.check(lib.skr_step_masked_backward_launch(ctypes.byref(plan), g.data_ptr(), ctypes.byref(desc), arr, numel, sample_numel, stream), "skr_step_masked_backward_launch"),
        "plain": lambda: _hip.check(lib.skr_step_backward_launch(ctypes.byref(plan), g.data_ptr(), None, arr, numel, stream), "skr_step_backward_launch"),
    }
    nbytes = {"masked": numel * 2 * (GRADS + 1) + mask.numel() * 2, "plain": numel * 2 * (GRADS + 1)}
    for launch in launches.values():
        for _ in range(WARMUP):
            launch()
    torch.cuda.synchronize()
    per = {name: [] for name in launches}
    for _ in range(args.repeats):
        for name, launch in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            per[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    lines = [f"masked backward: {BATCH} x {SHAPE} bf16, (B, 1, H, W) bf16 mask, {GRADS} gradients of one incoming gradient; {args.repeats} repeats of {args.launches} launches, "
             f"the two launches alternating in one process after {WARMUP} warm-up launches each  ({torch.cuda.get_device_name(0)})",
             "us per launch, event clock: median (min - max) over the repeats"]  # fmt: skip
    stats = {name: summary(values) for name, values in per.items()}
    for name, (m, lo, hi) in stats.items():
        lines.append(f"  {name:6s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})   {nbytes[name] / 1e6:7.1f} MB -> {nbytes[name] / (m * 1e-6) / PEAK * 100:5.1f} % of 8 TB/s")
    ratio, byte_ratio = stats["masked"][0] / stats["plain"][0], nbytes["masked"] / nbytes["plain"]
    spread = sum((hi - lo) / m for m, lo, hi in stats.values())
    lines.append(f"  masked / plain: {ratio:.3f} by the medians, {byte_ratio:.3f} by bytes; relative min - max spreads of the two together {spread:.3f}: the excess over the byte "
                 f"ratio ({ratio - byte_ratio:+.3f}) is {'larger than' if ratio - byte_ratio > spread else 'within'} the run-to-run spread")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
