"""Cost of one draw of the rolling generator entries against the whole-batch entries, through the C ABI: capacity 64 x (4, 128, 128) bf16,
Pyramid (defaults: strength 0.3, every level) and Offset (defaults: one offset per channel, strength 0.2).

  python tools/bench_rolling_noise.py [--repeats 7] [--draws 2000] [--out profiles/rolling_noise.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  whole-batch entry          skr_noise_pyramid / skr_noise_offset on 64 samples, one draw number for all: the yardstick, untouched code
  b  rolling, 64 of 64 active   skr_noise_pyramid_rolling / skr_noise_offset_rolling, every slot at a draw number of its own
  c  rolling, 16 of 64 active   the same, every fourth slot active: the other 48 samples' workgroups leave on their first scalar branch
The draw numbers move on with every call (form a: the batch's; b / c: every slot's own position, as a tick of a rolling batch does), so no
call repeats the previous one's streams.  Per repeat, `draws` calls are timed with HIP events (first enqueue to last kernel) after a
warm-up of 100 calls; reported per form: median and min - max over the repeats, us per draw.
Stated with the numbers: whether b is within the two forms' min - max spreads together of a, and whether c is below b by more than theirs."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CAPACITY, SHAPE, WARMUP, ROWS = 64, (4, 128, 128), 100, 1 << 20
GENERATORS = ("pyramid", "offset")
FORMS = {"a": "whole-batch entry", "b": "rolling, 64 of 64 active", "c": "rolling, 16 of 64 active"}


def child(generator: str, form: str, repeats: int, draws: int) -> None:
    import torch

    from skrample_amd import _hip
    from skrample_amd.pytorch import noise as N

    dev = torch.device("cuda:0")
    lib, stream = _hip.load(), _hip.current_stream_ptr(dev)
    seeds = torch.arange(1, CAPACITY + 1, dtype=torch.int64, device=dev)
    out = torch.empty((CAPACITY, *SHAPE), dtype=torch.bfloat16, device=dev)
    active = [b for b in range(CAPACITY) if form != "c" or b % 4 == 0]
    # one index vector per call, uploaded ahead of the timed region: slot b at position (call + b) of its own run
    total = WARMUP + repeats * draws
    slots = torch.arange(CAPACITY, dtype=torch.int64)
    live = torch.zeros(CAPACITY, dtype=torch.bool)
    live[active] = True
    index = torch.where(live[None, :], slots[None, :] * ROWS + (torch.arange(total, dtype=torch.int64)[:, None] + slots[None, :]) % ROWS, torch.full((1, 1), -1, dtype=torch.int64))
    index = index.to(torch.int32).to(dev)
    first, stride = index.data_ptr(), CAPACITY * index.element_size()  # (call n reads row n: no tensor indexing inside the timed loop)
    code = _hip.DTYPE_CODE[torch.bfloat16]
    if generator == "pyramid":
        props = N.PyramidProps()
        _, (lead, h, w, resize_h), _ = N.Pyramid._plan(SHAPE, props)
        scratch, levels, partials = N.Pyramid._lds_workspace(CAPACITY, lead * h * w, lead, dev)
        depth = int(min(props.depth, 1 << 20))

        def whole(n):
            return lib.skr_noise_pyramid(out.data_ptr(), code, scratch.data_ptr(), partials.data_ptr(), levels.data_ptr(), seeds.data_ptr(), n * N.SUBSTREAMS, n * N.SUBSTREAMS,
                                         CAPACITY, lead, h, w, resize_h, float(props.strength), depth, 1, stream)  # fmt: skip

        def rolling(n):
            return lib.skr_noise_pyramid_rolling(out.data_ptr(), code, scratch.data_ptr(), partials.data_ptr(), levels.data_ptr(), seeds.data_ptr(), first + n * stride, ROWS,
                                                 N.SUBSTREAMS, 0, CAPACITY, lead, h, w, resize_h, float(props.strength), depth, stream)  # fmt: skip
    else:
        props = N.OffsetProps()
        sizes, mask = N.Offset._merged(SHAPE, props)
        shape = (ctypes.c_int64 * len(sizes))(*sizes)

        def whole(n):
            return lib.skr_noise_offset(out.data_ptr(), code, seeds.data_ptr(), n * N.SUBSTREAMS, n * N.SUBSTREAMS + 1, CAPACITY, shape, len(sizes), mask, float(props.strength), stream)

        def rolling(n):
            return lib.skr_noise_offset_rolling(out.data_ptr(), code, seeds.data_ptr(), first + n * stride, ROWS, N.SUBSTREAMS, 0, CAPACITY, shape, len(sizes), mask,
                                                float(props.strength), stream)  # fmt: skip

    draw = whole if form == "a" else rolling
    n = 0
    for _ in range(WARMUP):
        _hip.check(draw(n), "draw")
        n += 1
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = 0
        for _ in range(draws):
            status |= draw(n)
            n += 1
        e1.record()
        torch.cuda.synchronize()
        _hip.check(status, "draw")
        event_us.append(e0.elapsed_time(e1) * 1e3 / draws)
    assert torch.isfinite(out[active].float()).all()
    print("RESULT " + json.dumps({"generator": generator, "form": form, "event_us": event_us, "device": torch.cuda.get_device_name(0)}), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--draws", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_noise.txt"))
    ap.add_argument("--child", nargs=2, metavar=("GENERATOR", "FORM"))
    args = ap.parse_args()
    if args.repeats < 5 or args.draws < 500:
        ap.error("at least 5 repeats of at least 500 draws")
    if args.child:
        child(args.child[0], args.child[1], args.repeats, args.draws)
        return 0
    lines = [f"rolling draws: capacity {CAPACITY} x {SHAPE} bf16 through the C ABI; {args.repeats} repeats of {args.draws} draws after {WARMUP} warm-up draws",
             "us per draw (HIP events): median (min - max) over the repeats; one child process per generator and form"]  # fmt: skip
    for generator in GENERATORS:
        seen = {}
        for form in FORMS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--draws", str(args.draws), "--child", generator, form],
                                 capture_output=True, text=True, timeout=600)  # fmt: skip
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"{generator} / form {form} failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[form] = json.loads(found[-1][len("RESULT "):])
        lines.append(f"{generator}  ({seen['a']['device']})")
        stats = {form: summary(seen[form]["event_us"]) for form in FORMS}
        for form, what in FORMS.items():
            m, lo, hi = stats[form]
            lines.append(f"  {form}  {what:26s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
        spread = lambda form: stats[form][2] - stats[form][1]  # noqa: E731
        ab, bc = stats["b"][0] - stats["a"][0], stats["b"][0] - stats["c"][0]
        lines.append(f"  b - a = {ab:+.2f} us ({100 * ab / stats['a'][0]:+.1f} %), the two spreads together {spread('a') + spread('b'):.2f} us: b is "
                     f"{'within' if abs(ab) <= spread('a') + spread('b') else ('slower than a beyond' if ab > 0 else 'faster than a beyond')} the spreads")  # fmt: skip
        lines.append(f"  b - c = {bc:+.2f} us (c is {stats['c'][0] / stats['b'][0]:.2f} of b with a quarter of the slots active), the two spreads together {spread('b') + spread('c'):.2f} us: c is "
                     f"{'below b by more than' if bc > spread('b') + spread('c') else 'NOT below b by more than'} the spreads")  # fmt: skip
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
