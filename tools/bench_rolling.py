"""Cost of rolling launches: skr_step_launch_indexed_per_sample (the yardstick: its kernels are the parent commit's) against
skr_step_launch_rolling, through the C ABI, alternating in one process on rotating buffer sets larger than the Infinity Cache.

  python tools/bench_rolling.py [rounds]     # default 5 rounds of A B C D per case

Cases: the headline launch (256x4x128x128 bf16, DPM-2 SDE: 4 operands + Philox), a UniPC-3 launch with two outputs (8 bf16 + 1 fp32
operands, Philox on both), one Runge-Kutta stage (4 operands, rounded pair conversion).  Per case and round, in this order:
  A  per-sample launch, 256 distinct rows                       (the yardstick)
  B  rolling launch, every slot active, every operand present   (cost of the row fetch in front of the loads)
  C  rolling launch, every second slot inactive                 (must be faster than A: it moves half the bytes)
  D  rolling launch, every fourth sample at position 0          (only this tick's sample and model output present there;
                                                                 not for the Runge-Kutta stage, which has no ramp-up)
Printed: us per launch of every round (HIP events over `iters` launches after conditioning), then per form the median, the ratio
of medians to A with A's own run-to-run spread ((max - min) / median over the rounds) beside it -- a ratio inside that spread is no
measured difference -- and the time the form's algorithmic bytes take at 8 TB/s."""

import ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from skrample_amd import _hip
from skrample_amd.sampling.lazy import empty_output

dev = torch.device("cuda:0")
lib = _hip.load()
stream = torch.cuda.current_stream(dev).cuda_stream
BATCH, SAMPLE = 256, 4 * 128 * 128


def case(name, n_a, n_b, two_out, noise, rk, rounds, iters=200, footprint=1.2e9):
    n = BATCH * SAMPLE
    dtype, item = torch.bfloat16, 2
    per_set = n * (n_a * item + n_b * 4 + (4 + item if two_out else item) + (item if rk else 0))
    nsets = max(2, min(8, int(footprint // per_set) + 1))
    g = torch.Generator(device=dev).manual_seed(1)

    def alloc(dt, engine_owned, fill=True):  # (placement as in tools/bench_plan.py: engine results from the engine's allocator)
        t = empty_output((n,), dt, dev) if engine_owned else torch.empty(n, device=dev, dtype=dt)
        if fill:
            t.copy_(torch.randn(n, device=dev, generator=g))
        return t

    calls, keep = [], []
    for _ in range(nsets):
        ins = [alloc(dtype, k % 2 == 0) for k in range(n_a)] + [alloc(torch.float32, True) for _ in range(n_b)]
        o0 = alloc(torch.float32 if two_out else dtype, True, fill=False)
        o1 = alloc(dtype, True, fill=False) if (two_out or rk) else None
        keep.append((ins, o0, o1))
        calls.append(((ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins]), o0.data_ptr(), o1.data_ptr() if o1 is not None else None))
    seeds = torch.arange(BATCH, dtype=torch.int64, device=dev) + 42
    code = _hip.DTYPE_CODE[dtype]
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b = n_a + n_b, n_a, code, _hip.F32 if n_b else code
    plan.out0_dtype = _hip.F32 if two_out else code
    plan.out1_dtype = code if (two_out or rk) else -1
    plan.sample_numel, plan.noise_mode = SAMPLE, 1 if noise else 0
    if rk:
        plan.convert_to, plan.convert_from = 1, 1
    rows = (_hip.StepRowC * (BATCH + 1))()
    for r, row in enumerate(rows):  # 256 rows that differ a little (a real table: other sigmas per request)
        for k in range(n_a + n_b):
            row.coef0[k], row.coef1[k] = 0.1 * (k + 1) + 1e-4 * r, -0.05 * (k + 1) - 1e-4 * r
        row.chain = 0.5
        if noise:
            row.zeta0, row.zeta1, row.stream0, row.stream1 = 0.3 + 1e-4 * r, (0.2 if two_out else 0.0), 1, 2
        for i, v in enumerate((0.7, 0.9, 0.4, 1.3)):
            row.convert_k[i] = v
    for k in range(2, n_a + n_b):  # row 256: a sample at position 0 of its run -- no history, no state
        rows[BATCH].coef0[k] = rows[BATCH].coef1[k] = 0.0
    rows_dev = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    distinct = torch.arange(BATCH, dtype=torch.int32, device=dev)
    half = torch.where(distinct % 2 == 0, distinct, torch.full_like(distinct, -1))
    fresh = torch.where(distinct % 4 == 0, torch.full_like(distinct, BATCH), distinct)
    seeds_ptr = seeds.data_ptr() if noise else None
    rolling = lambda index: lambda ptrs, p0, p1: lib.skr_step_launch_rolling(ctypes.byref(plan), ptrs, p0, p1, seeds_ptr, n, rows_dev.data_ptr(), index.data_ptr(), 0, stream)  # noqa: E731
    forms = {
        "A per-sample": lambda ptrs, p0, p1: lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), ptrs, p0, p1, seeds_ptr, n, rows_dev.data_ptr(), distinct.data_ptr(), 0, stream),
        "B rolling, full": rolling(distinct),
        "C rolling, half inactive": rolling(half),
    }  # fmt: skip
    if not rk:
        forms["D rolling, quarter at 0"] = rolling(fresh)
    in_bytes = [item] * n_a + [4] * n_b
    out_bytes = (4 + item if two_out else item) + (item if rk else 0)
    full = SAMPLE * (sum(in_bytes) + out_bytes)
    algorithmic = {"A per-sample": BATCH * full, "B rolling, full": BATCH * full, "C rolling, half inactive": BATCH // 2 * full,
                   "D rolling, quarter at 0": BATCH * 3 // 4 * full + BATCH // 4 * SAMPLE * (sum(in_bytes[:2]) + out_bytes)}  # fmt: skip

    def run(form, count):
        for i in range(count):
            st = form(*calls[i % nsets])
            if st:
                _hip.check(st, "launch")

    def timed(form, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(form, count); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / count

    # conditioning: the launch time of a sustained run settles only after ~16 ms ("Launch time over a long run")
    us = timed(forms["A per-sample"], 20)
    for form in forms.values():
        run(form, int(10e3 / max(us, 1.0)) + 1)
    torch.cuda.synchronize()
    seen = {k: [] for k in forms}
    for _ in range(rounds):
        for key, form in forms.items():
            run(form, 20)
            torch.cuda.synchronize()
            seen[key].append(timed(form, iters))
    print(f"{name}  ({per_set / 1e6:.0f} MB per launch, {nsets} buffer sets)")
    base = statistics.median(seen["A per-sample"])
    spread = (max(seen["A per-sample"]) - min(seen["A per-sample"])) / base
    for key, vals in seen.items():
        med = statistics.median(vals)
        tail = f"spread of A {spread * 100:.2f} %" if key.startswith("A") else f"ratio to A {med / base:.4f}"
        print(f"  {key:26s} " + " ".join(f"{v:7.2f}" for v in vals) + f"  us   median {med:7.2f}   {tail}   bytes / 8 TB/s {algorithmic[key] / 8e6:6.2f} us", flush=True)
    del keep


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    case("headline: DPM-2 SDE, 4 bf16 operands + Philox -> bf16", 4, 0, False, True, False, rounds)
    case("UniPC-3: 8 bf16 + 1 fp32 operands + Philox -> fp32 + bf16", 8, 1, True, True, False, rounds)
    case("Runge-Kutta stage: 4 bf16 operands, rounded conversion -> 2 x bf16", 4, 0, False, False, True, rounds)
