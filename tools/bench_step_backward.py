"""Time the transposed step (skr_step_backward_launch) at the headline shape, 256x4x128x128.

  dpm2        one bf16 incoming gradient, four bf16 operand gradients: 1 read + 4 writes (one-trip kernel)
  unipc3      two bf16 incoming gradients (corrector out0 + predictor out1), five bf16 operand gradients: 2 reads + 5 writes (one-trip kernel)
  dpm2_mixed  one fp32 incoming gradient (a step whose output is in compute_scale=float32) and four bf16 operand gradients: the mixed-dtype
              case, which the grid-stride kernel serves

Every case rotates over enough buffer sets (incoming gradients and operand gradients alike) that one pass touches more than 1 GB, four
times the 256 MiB Infinity Cache, so the numbers are HBM numbers, as bench.py's.  For each: microseconds per launch, achieved bandwidth as
a fraction of the 8 TB/s spec, and the time of what it replaces on the same rotating buffers -- per operand one torch `mul` (one incoming
gradient) or one `mul` plus one `add` with alpha (two).  One JSON line per case.

    python tools/bench_step_backward.py [--iters 200] [--reps 5] [--footprint-gb 1.1]
"""

import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from skrample_amd import _hip  # noqa: E402

SHAPE = (256, 4, 128, 128)
PEAK_GBS = 8000.0
CASES = (("dpm2", 1, 4, torch.bfloat16), ("unipc3", 2, 5, torch.bfloat16), ("dpm2_mixed", 1, 4, torch.float32))


def timed(fn, n_sets: int, iters: int, reps: int) -> float:
    "best of `reps` averages over `iters` back-to-back calls on rotating buffer sets, microseconds"
    for i in range(2 * n_sets):
        fn(i % n_sets)
    best = float("inf")
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(iters):
            fn(i % n_sets)
        end.record()
        end.synchronize()
        best = min(best, start.elapsed_time(end) * 1e3 / iters)
    return best


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--footprint-gb", type=float, default=1.1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _hip.load()
    numel = math.prod(SHAPE)
    stream = _hip.current_stream_ptr(dev)
    for name, n_in, n_out, g_dtype in CASES:
        set_bytes = numel * (n_in * torch.finfo(g_dtype).bits // 8 + n_out * 2)
        n_sets = max(2, math.ceil(args.footprint_gb * 1e9 / set_bytes))
        gs = [[torch.randn(SHAPE, device=dev).to(g_dtype) for _ in range(n_in)] for _ in range(n_sets)]
        outs = [[torch.empty(SHAPE, device=dev, dtype=torch.bfloat16) for _ in range(n_out)] for _ in range(n_sets)]
        a = [0.5 + 0.1 * k for k in range(n_out)]
        b = [-0.3 + 0.05 * k for k in range(n_out)]
        plan = _hip.StepGradPlanC()
        plan.n_grads, plan.n_group_a, plan.dtype_a, plan.dtype_b = n_out, n_out, _hip.BF16, _hip.BF16
        plan.g0_dtype = _hip.DTYPE_CODE[g_dtype]
        plan.g1_dtype = _hip.DTYPE_CODE[g_dtype] if n_in == 2 else _hip.NONE
        for k in range(n_out):
            plan.a[k], plan.b[k] = a[k], b[k]
        ptrs = [(gs[s][0].data_ptr(), gs[s][1].data_ptr() if n_in == 2 else None, (ctypes.c_void_p * n_out)(*[t.data_ptr() for t in outs[s]])) for s in range(n_sets)]

        def kernel(s):
            g0, g1, arr = ptrs[s]
            _hip.check(lib.skr_step_backward_launch(ctypes.byref(plan), g0, g1, arr, numel, stream), "skr_step_backward_launch")

        def torch_ops(s):
            for k in range(n_out):
                torch.mul(gs[s][0], a[k], out=outs[s][k])
                if n_in == 2:
                    outs[s][k].add_(gs[s][1], alpha=b[k])

        us = timed(kernel, n_sets, args.iters, args.reps)
        us_torch = timed(torch_ops, n_sets, max(args.iters // 4, 2 * n_sets), args.reps)
        gbs = set_bytes / (us * 1e-6) / 1e9
        print(json.dumps({"case": name, "shape": list(SHAPE), "grad_in_dtype": str(g_dtype).split(".")[-1], "grad_out_dtype": "bfloat16", "reads": n_in, "writes": n_out,
                          "bytes": set_bytes, "buffer_sets": n_sets, "footprint_bytes": set_bytes * n_sets, "us": round(us, 2), "gb_s": round(gbs, 1),
                          "frac_of_8tb": round(gbs / PEAK_GBS, 3), "torch_ops_us": round(us_torch, 2), "speedup_vs_torch_ops": round(us_torch / us, 2)}), flush=True)
        del gs, outs, ptrs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
