"""Host cost of enqueueing a colored draw: wall time of a loop of `skr_noise_colored` / `skr_noise_colored_any` calls with no
synchronisation inside (one after), per call.  The units are small, so that the GPU drains the queue faster than the host fills it
and the loop measures the launchers' own dispatch -- route decision, `hipFuncSetAttribute`, `getenv`, the launches.

    python tools/bench_colored_dispatch.py                       # the library SKR_HIP_LIB names, else the in-tree one: one JSON line
    python tools/bench_colored_dispatch.py --ab OLD.so NEW.so    # A/B: fresh processes, alternating, --rounds each (default 3)

Per process and unit: the median over --loops loops (default 15) of --calls calls (default 200), in microseconds per call.  --ab
prints every process's medians, then per unit the median of each library's medians, their difference and the old library's own
spread (max - min of its medians): a difference inside that spread is one the machine cannot resolve."""
import argparse, ctypes, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ((2, 8, 16), (2, 12, 24), (8, 128, 256), (3, 8, 16))  # fused planes, mixed planes, separate passes, colored_planes through skr_noise_colored_any
BATCH = 2


def measure(calls: int, loops: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    from skrample_amd import _hip
    from skrample_amd.pytorch import noise as PN

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
        for _ in range(50):
            assert call() == 0, unit
        torch.cuda.synchronize()
        per_call = []
        for _ in range(loops):
            t0 = time.perf_counter()
            for _ in range(calls):
                call()
            per_call.append((time.perf_counter() - t0) / calls * 1e6)
            torch.cuda.synchronize()
        out["x".join(map(str, unit))] = round(statistics.median(per_call), 3)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ab", nargs=2, metavar=("OLD_LIB", "NEW_LIB"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--loops", type=int, default=15)
    a = ap.parse_args()
    if not a.ab:
        print(json.dumps({"lib": os.environ.get("SKR_HIP_LIB", "in-tree"), "us_per_call": measure(a.calls, a.loops)}))
        return 0
    runs = {"old": [], "new": []}
    for r in range(a.rounds):
        for side, lib in zip(("old", "new"), a.ab):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--loops", str(a.loops)], env={**os.environ, "SKR_HIP_LIB": os.path.abspath(lib)},
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print(p.stdout, p.stderr, sep="\n")
                return 1
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1])["us_per_call"])
            print(f"round {r + 1} {side}: {runs[side][-1]}", flush=True)
    print("unit          old median  new median  new - old  old spread (max - min)   [us per call]")
    inside = True
    for unit in runs["old"][0]:
        old, new = [x[unit] for x in runs["old"]], [x[unit] for x in runs["new"]]
        mo, mn, spread = statistics.median(old), statistics.median(new), max(old) - min(old)
        inside &= mn - mo <= spread
        print(f"{unit:<13} {mo:10.3f}  {mn:10.3f}  {mn - mo:+9.3f}  {spread:10.3f}   {'inside' if mn - mo <= spread else 'OUTSIDE'}")
    return 0 if inside else 2


if __name__ == "__main__":
    sys.exit(main())
