"""Cost of a guided in-painting step in one launch against the two launches it replaces, through the C ABI: 64 x (4, 128, 128) bf16
latents, masks (64, 1, 128, 128), the DPM-2 plan of a middle step as the sampler emits it (lifted from a wrapper run through _hip.trace).

  python tools/bench_guided_masked.py [--repeats 7] [--launches 2000] [--out profiles/guided_masked.txt]

Forms, each in a child process of its own (a fresh HIP context and allocator per form; the parent never opens the GPU):
  a  the two launches   the guidance-only form of skr_step_launch_guided, which writes the prediction, then skr_step_launch_masked over
                        the operand list with that tensor in the slot: the yardstick, untouched code
  b  the one launch     skr_guided_masked_step_launch
Both again with guidance_rescale 0.7: skr_guidance_rescale_factor in front on both sides, the rescaled guidance-only launch in a.
Per repeat, `launches` steps are timed with HIP events (first enqueue to last kernel) after a warm-up of 100; reported per form: median and
min - max over the repeats, us per step.  Stated with the numbers: whether b is below a by more than the two min - max spreads together.
The operands of one step are 8 tensors of 8 MiB: they stay resident in the last-level cache between steps, for both forms alike."""

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCH, SHAPE, WARMUP, SCALE, PHI = 64, (4, 128, 128), 100, 7.5, 0.7
FORMS = {"a": "the two launches", "b": "the one launch"}


def child(form: str, phi: float, repeats: int, launches: int) -> None:
    import torch

    import skrample_amd.diffusers as PD
    import skrample_amd.scheduling as PS
    from skrample_amd import _hip
    from skrample_amd.sampling import structured as PT

    dev = torch.device("cuda:0")
    lib, stream = _hip.load(), _hip.current_stream_ptr(dev)
    g = torch.Generator().manual_seed(1)
    normal = lambda: torch.randn((BATCH, *SHAPE), generator=g).bfloat16().to(dev)  # noqa: E731
    # the plan of a middle step, as the sampler emits it: the fifth of ten steps of a wrapper run, its one launch read off the trace
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    w.set_timesteps(10)
    w.set_inpaint(torch.rand((BATCH, 1, *SHAPE[1:]), generator=g).to(dev), normal(), normal(), fuse_guidance=True)
    x = normal()
    for i, t in enumerate(w.timesteps.tolist()[:5]):
        _hip.trace = []
        try:
            x = w.step_guided(normal(), normal(), SCALE, t, x, return_dict=False)[0]
            trace = list(_hip.trace)
        finally:
            _hip.trace = None
    (call,) = [e for e in trace if e.kind == "guided_masked"]
    plan, ops, numel, slot = call.plan, list(call.inputs), call.numel, call.slot
    sample_numel = numel // BATCH
    out, p, factor = torch.empty_like(x), torch.empty_like(x), torch.empty(BATCH, dtype=torch.bfloat16, device=dev)
    partials = torch.empty(_hip.guidance_partials(numel, sample_numel), dtype=torch.float64, device=dev)
    array = lambda tensors: (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])  # noqa: E731
    only = _hip.StepPlanC()
    only.n_terms = only.n_group_a = 1
    only.dtype_a = only.dtype_b = _hip.BF16
    only.out0_dtype = only.out1_dtype = _hip.NONE
    only.coef0[0] = 1.0
    mask = _hip.StepMaskC(call.mask.data_ptr(), _hip.BF16, 0, call.mask_numel, call.batch_stride)
    rescale = _hip.StepRescaleC(factor.data_ptr(), phi, sample_numel, 0)
    guide_only = _hip.StepGuidanceC(call.cond.data_ptr(), p.data_ptr(), SCALE, 0, 0)
    guide = _hip.StepGuidanceC(call.cond.data_ptr(), p.data_ptr(), SCALE, slot, 0)
    uncond, with_p = array([ops[slot]]), array(ops[:slot] + [p] + ops[slot + 1 :])
    operands, by = array(ops), ctypes.byref
    statistic = (lib.skr_guidance_rescale_factor, (ops[slot].data_ptr(), call.cond.data_ptr(), _hip.BF16, SCALE, numel, sample_numel, factor.data_ptr(), None, partials.data_ptr(), stream))
    if form == "a":
        first = (lib.skr_step_launch_guided_rescaled, (by(only), uncond, None, by(guide_only), by(rescale), None, numel, stream)) if phi else (
            lib.skr_step_launch_guided, (by(only), uncond, None, by(guide_only), None, numel, stream))
        step = [first, (lib.skr_step_launch_masked, (by(plan), with_p, out.data_ptr(), by(mask), None, numel, stream))]
    else:
        step = [(lib.skr_guided_masked_step_launch, (by(plan), operands, out.data_ptr(), by(guide), by(rescale) if phi else None, by(mask), None, numel, stream))]
    if phi:
        step.insert(0, statistic)
    assert plan.noise_mode == 0  # (DPM-2 draws nothing)

    def run(count):
        status = 0
        for _ in range(count):
            for entry, args in step:
                status |= entry(*args)
        return status

    _hip.check(run(WARMUP), "warm-up")
    torch.cuda.synchronize()
    event_us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = run(launches)
        e1.record()
        torch.cuda.synchronize()
        _hip.check(status, "step")
        event_us.append(e0.elapsed_time(e1) * 1e3 / launches)
    assert torch.isfinite(out.float()).all() and torch.isfinite(p.float()).all()
    digest = [int(out.view(torch.int16).to(torch.int64).sum()), int(p.view(torch.int16).to(torch.int64).sum())]  # (equal for a and b: the bit contract, seen once more)
    print("RESULT " + json.dumps({"form": form, "phi": phi, "n_terms": plan.n_terms, "event_us": event_us, "digest": digest, "device": torch.cuda.get_device_name(0)}), flush=True)


def summary(values):
    return statistics.median(values), min(values), max(values)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_masked.txt"))
    ap.add_argument("--child", nargs=2, metavar=("FORM", "PHI"))
    args = ap.parse_args()
    if args.repeats < 5 or args.launches < 500:
        ap.error("at least 5 repeats of at least 500 launches")
    if args.child:
        child(args.child[0], float(args.child[1]), args.repeats, args.launches)
        return 0
    lines = [f"guided in-painting step: {BATCH} x {SHAPE} bf16, masks ({BATCH}, 1, {SHAPE[1]}, {SHAPE[2]}), DPM-2 plan of a middle step through the C ABI; "
             f"{args.repeats} repeats of {args.launches} steps after {WARMUP} warm-up steps",
             "us per step (HIP events): median (min - max) over the repeats; one child process per form"]  # fmt: skip
    for phi in (0.0, PHI):
        seen = {}
        for form in FORMS:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--launches", str(args.launches), "--child", form, str(phi)],
                                 capture_output=True, text=True, timeout=600)  # fmt: skip
            found = [line for line in run.stdout.splitlines() if line.startswith("RESULT ")]
            if run.returncode != 0 or not found:
                sys.stderr.write(run.stdout[-2000:] + run.stderr[-4000:])
                print(f"form {form}, guidance_rescale {phi} failed with exit status {run.returncode}: stopping", file=sys.stderr)
                return 1  # (nothing more is started on the device after a failure)
            seen[form] = json.loads(found[-1][len("RESULT "):])
        lines.append(f"guidance_rescale {phi}: {seen['a']['n_terms']} operands  ({seen['a']['device']})" + (", the statistics launch in front on both sides" if phi else ""))
        stats = {form: summary(seen[form]["event_us"]) for form in FORMS}
        for form, what in FORMS.items():
            m, lo, hi = stats[form]
            lines.append(f"  {form}  {what:18s} {m:8.2f} ({lo:8.2f} - {hi:8.2f})")
        spreads = sum(stats[form][2] - stats[form][1] for form in FORMS)
        gain = stats["a"][0] - stats["b"][0]
        lines.append(f"  a - b = {gain:+.2f} us ({100 * gain / stats['a'][0]:+.1f} % of a), the two spreads together {spreads:.2f} us: b is "
                     f"{'below a by more than' if gain > spreads else 'NOT below a by more than'} the spreads; outputs of a and b "
                     f"{'equal' if seen['a']['digest'] == seen['b']['digest'] else 'DIFFER'} (sums of their bits)")  # fmt: skip
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
