"""Host cost of enqueueing a launch: wall time of a loop of calls of one entry point with no synchronisation inside (one after), per
call.  The units are small, so that the GPU drains the queue faster than the host fills it and the loop measures the launchers' own
dispatch -- checks, route decision, dtype dispatch, `hipFuncSetAttribute`, `getenv`, the launches.  Three unit sets: colored draws
(`skr_noise_colored` / `skr_noise_colored_any`, the default; the tool is named after them), the step family and Pyramid draws.

    python tools/bench_colored_dispatch.py                       # the library SKR_HIP_LIB names, else the in-tree one: one JSON line
    python tools/bench_colored_dispatch.py --ab OLD.so NEW.so    # A/B: fresh processes, alternating, --rounds each (default 3)
    python tools/bench_colored_dispatch.py --units step ...      # the step family instead: one small launch each of skr_step_launch (bf16,
                                                                 # 4 operands, one chunk per sample), the masked and the backward launch,
                                                                 # skr_power_blend and skr_error_mean
    python tools/bench_colored_dispatch.py --units pyramid ...   # Pyramid draws, a unit per arm: generic, strip / 256, UNI (LDS opt-in), a
                                                                 # width skr_noise_pyramid refuses followed by skr_noise_pyramid_any (what
                                                                 # the Python layer does at such a shape's first draw), skr_noise_pyramid_nd

Per process and unit: the median over --loops loops (default 15) of --calls calls (default 200), in microseconds per call.  --ab
prints every process's medians, then per unit the median of each library's medians, their difference and the old library's own
spread (max - min of its medians): a difference inside that spread is one the machine cannot resolve."""
import argparse, ctypes, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ((2, 8, 16), (2, 12, 24), (8, 128, 256), (3, 8, 16))  # fused planes, mixed planes, separate passes, colored_planes through skr_noise_colored_any
BATCH = 2


def timed(call, what, calls: int, loops: int) -> float:
    import torch

    for _ in range(50):
        assert call() == 0, what
    torch.cuda.synchronize()
    per_call = []
    for _ in range(loops):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        per_call.append((time.perf_counter() - t0) / calls * 1e6)
        torch.cuda.synchronize()
    return round(statistics.median(per_call), 3)


def step_calls() -> dict:
    "{unit: call} of the step family: 2 samples of one 2048-element chunk, bf16"
    import torch
    from skrample_amd import _hip

    lib, dev = _hip.load(), torch.device("cuda:0")
    n, numel = 4, 2 * 2048
    ops = [torch.randn(numel, device=dev).bfloat16() for _ in range(n)]
    out, mask = torch.empty(numel, dtype=torch.bfloat16, device=dev), torch.rand(2048, device=dev).bfloat16()
    grads = [torch.empty(numel, dtype=torch.bfloat16, device=dev) for _ in range(n)]
    wide, mean, partials = torch.empty(numel, device=dev), torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1024, dtype=torch.float64, device=dev)
    st = _hip.current_stream_ptr(dev)
    arr, garr = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in (ops, grads))
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = plan.out0_dtype = _hip.BF16
    plan.dtype_b, plan.out1_dtype, plan.sample_numel = _hip.F32, _hip.NONE, 2048
    gplan = _hip.StepGradPlanC()
    gplan.n_grads = gplan.n_group_a = n
    gplan.dtype_a = gplan.g0_dtype = _hip.BF16
    gplan.dtype_b, gplan.g1_dtype = _hip.F32, _hip.NONE
    for k in range(n):
        plan.coef0[k], plan.coef1[k], gplan.a[k] = 0.5 + k, 0.25 * (k % 2), 0.5 + k
    desc = _hip.StepMaskC(mask.data_ptr(), _hip.BF16, 0, 2048, 0)
    return {
        "step": lambda: lib.skr_step_launch(ctypes.byref(plan), arr, out.data_ptr(), None, None, numel, st),
        "masked": lambda: lib.skr_step_launch_masked(ctypes.byref(plan), arr, out.data_ptr(), ctypes.byref(desc), None, numel, st),
        "backward": lambda: lib.skr_step_backward_launch(ctypes.byref(gplan), ops[0].data_ptr(), None, garr, numel, st),
        "power_blend": lambda: lib.skr_power_blend(wide.data_ptr(), _hip.F32, ops[0].data_ptr(), _hip.BF16, ops[1].data_ptr(), _hip.BF16, 0.5, 0.5, 2.0, numel, st),
        "error_mean": lambda: lib.skr_error_mean(ops[0].data_ptr(), ops[1].data_ptr(), _hip.BF16, numel, 2, mean.data_ptr(), partials.data_ptr(), st),
    }


def pyramid_calls() -> dict:
    "{unit: call} of the Pyramid entry points: 2 samples, bf16"
    import torch
    from skrample_amd import _hip
    from skrample_amd.pytorch import noise as PN

    lib, dev = _hip.load(), torch.device("cuda:0")
    st, seeds = _hip.current_stream_ptr(dev), PN.seeds_tensor([7, 8], dev)
    def calls_of(unit):
        "the calls that draw `unit` = (lead, h, w), or its axes 0 and 2, into buffers of their own"
        n = unit[0] * unit[1] * unit[2]
        res = torch.empty((BATCH, *unit), dtype=torch.bfloat16, device=dev)
        scratch, normals = (torch.empty(BATCH * n, dtype=torch.float32, device=dev) for _ in range(2))
        partials = torch.empty(BATCH * unit[0] * 2, dtype=torch.float64, device=dev)  # (a pair per leading slice; the any-shape calls ask for one slot)
        table = torch.empty(BATCH * 17, dtype=torch.int32, device=dev)
        shape = (ctypes.c_int64 * 3)(*unit)
        head, tail = (res.data_ptr(), _hip.BF16, scratch.data_ptr()), (table.data_ptr(), seeds.data_ptr(), 0, 0, BATCH)

        def lds():
            return lib.skr_noise_pyramid(*head, partials.data_ptr(), *tail, *unit, 1, 0.3, 99, 1, st)

        def any_shape():
            return lib.skr_noise_pyramid_any(*head, normals.data_ptr(), partials.data_ptr(), 1, *tail, *unit, 1, 0.3, 99, 1, st)

        def refused():
            return any_shape() if lds() == _hip.SKR_ERR_UNSUPPORTED else -1

        def nd():
            return lib.skr_noise_pyramid_nd(*head, normals.data_ptr(), partials.data_ptr(), 1, *tail, 3, shape, 0, 2, 0.3, 99, 1, st)

        return {"lds": lds, "refused": refused, "nd": nd}

    units = (("generic 1x16x16", (1, 16, 16), "lds"), ("strip256 1x96x128", (1, 96, 128), "lds"), ("uni 1x192x256", (1, 192, 256), "lds"), ("refused 1x30x90", (1, 30, 90), "refused"), ("nd 8x3x16 (0,2)", (8, 3, 16), "nd"))
    return {name: calls_of(unit)[which] for name, unit, which in units}


def measure(calls: int, loops: int, units: str = "colored") -> dict:
    sys.path.insert(0, ROOT)
    import torch
    from skrample_amd import _hip
    from skrample_amd.pytorch import noise as PN

    if units == "step":
        return {name: timed(call, name, calls, loops) for name, call in step_calls().items()}
    if units == "pyramid":
        return {name: timed(call, name, calls, loops) for name, call in pyramid_calls().items()}
    lib, dev = _hip.load(), torch.device("cuda:0")
    out = {}
    for unit in UNITS:
        n = unit[0] * unit[1] * unit[2]
        spec = torch.empty(BATCH * n // unit[2] * (unit[2] // 2 + 1), dtype=torch.complex64, device=dev)
        scratch = torch.empty(BATCH * n, dtype=torch.float32, device=dev)
        partials = torch.empty(4 * BATCH * 256, dtype=torch.float64, device=dev)
        res = torch.empty((BATCH, *unit), dtype=torch.bfloat16, device=dev)
        seeds = PN.seeds_tensor([7, 8], dev)
        st = _hip.current_stream_ptr(dev)
        dims = (ctypes.c_int32 * 3)(*unit)
        if unit[0] & (unit[0] - 1):
            def call():
                return lib.skr_noise_colored_any(res.data_ptr(), _hip.BF16, spec.data_ptr(), scratch.data_ptr(), partials.data_ptr(), seeds.data_ptr(), 512, BATCH, 3, dims, 1.0, 0, 0.0, st)
        else:
            def call():
                return lib.skr_noise_colored(res.data_ptr(), _hip.BF16, spec.data_ptr(), scratch.data_ptr(), partials.data_ptr(), 256, seeds.data_ptr(), 512, BATCH, *unit, 1.0, 0, 0.0, st)
        out["x".join(map(str, unit))] = timed(call, unit, calls, loops)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ab", nargs=2, metavar=("OLD_LIB", "NEW_LIB"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--loops", type=int, default=15)
    ap.add_argument("--units", choices=("colored", "step", "pyramid"), default="colored")
    a = ap.parse_args()
    if not a.ab:
        print(json.dumps({"lib": os.environ.get("SKR_HIP_LIB", "in-tree"), "us_per_call": measure(a.calls, a.loops, a.units)}))
        return 0
    runs = {"old": [], "new": []}
    for r in range(a.rounds):
        for side, lib in zip(("old", "new"), a.ab):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--loops", str(a.loops), "--units", a.units], env={**os.environ, "SKR_HIP_LIB": os.path.abspath(lib)},
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print(p.stdout, p.stderr, sep="\n")
                return 1
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1])["us_per_call"])
            print(f"round {r + 1} {side}: {runs[side][-1]}", flush=True)
    print("unit              old median  new median  new - old  old spread (max - min)   [us per call]")
    inside = True
    for unit in runs["old"][0]:
        old, new = [x[unit] for x in runs["old"]], [x[unit] for x in runs["new"]]
        mo, mn, spread = statistics.median(old), statistics.median(new), max(old) - min(old)
        inside &= mn - mo <= spread
        print(f"{unit:<17} {mo:10.3f}  {mn:10.3f}  {mn - mo:+9.3f}  {spread:10.3f}   {'inside' if mn - mo <= spread else 'OUTSIDE'}")
    return 0 if inside else 2


if __name__ == "__main__":
    sys.exit(main())
