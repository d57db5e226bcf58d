"""Operand views: the builders, the matrix and the paired runs shared by tests/test_operand_views_gpu.py and
tests/test_operand_views_host.py.

The contract under test, for every public entry point f and every view v of values V:
  (1) same bits as the contiguous run: f(v) has the bits of f(c), c a fresh, contiguous, 16-byte-aligned clone of the same values
      handed to a second wrapper / sampler in the same state -- for every result of the call and of all later steps of the run;
  (2) or a documented refusal that changes nothing (only the entries of REFUSES);
  (3) the caller's storage is untouched: every view lives in a larger base allocation with >= PAD elements of padding on each side,
      and the WHOLE base -- padding and the skipped elements of a strided slice included -- is bitwise what it was;
  (4) outputs are the engine's own: no result overlaps an operand's base, a result is contiguous, and it is channels-last exactly when
      every operand of the step shares one dense channels-last layout (never when some operand of the call does not).

Every kind is a function (values, base_filler) -> view with `values`' shape, dtype and numbers.  The base is filled with
`base_filler` (NaN by default: an element read outside the view shows up in the result) before the values are written through
the view."""

from __future__ import annotations

import torch

PAD = 64  # elements of padding on each side of every view
NAN = float("nan")
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
SHAPES = [(2, 4, 5, 7), (2, 4, 16, 16), (2, 8, 32, 32)]
# ^ (2,4,5,7): ragged everywhere -- a sample is 140 elements, numel % 8 != 0, in-kernel Philox not fusable; (2,4,16,16): whole vectors,
#   Philox fusable; (2,8,32,32): 16384 elements, more than one trip of a workgroup, channels-last plane >= 1024
CHUNK_SHAPE = (1, 4, 5, 7)  # the classifier-free-guidance idiom on a 280-byte bf16 sample: `cond` sits at an address that is 8 mod 16


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def _flat(n: int, like: torch.Tensor, filler: float) -> torch.Tensor:
    base = torch.full((n,), filler, dtype=like.dtype, device=like.device)
    assert base.data_ptr() % 16 == 0, "the allocator hands out 16-byte aligned blocks: the builders' address arithmetic relies on it"
    return base


def _channels_last_strides(shape) -> tuple:
    n, c, h, w = shape
    return (h * w * c, 1, w * c, c)


def _window(values: torch.Tensor, filler: float, shift: int) -> torch.Tensor:
    n = values.numel()
    base = _flat(PAD + shift + n + PAD, values, filler)
    view = base[PAD + shift : PAD + shift + n].view(values.shape)
    view.copy_(values)
    return view


def plain(values, filler=NAN):
    "control: contiguous and aligned, but still a window of a padded base"
    return _window(values, filler, 0)


def offset_small(values, filler=NAN):
    "the view starts one element into an aligned window: address = 2 mod 16 for 16-bit types, 4 for fp32, 8 for fp64"
    return _window(values, filler, 1)


def offset_8(values, filler=NAN):
    "address = 8 mod 16: what `& 15` catches and `& 7` would not"
    return _window(values, filler, 8 // values.element_size())


def chunk_second(values, filler=NAN):
    "`uncond, cond = doubled.chunk(2)`: the second half of a doubled batch (the first half holds the filler)"
    n = values.numel()
    base = _flat(PAD + 2 * n + PAD, values, filler)
    doubled = base[PAD : PAD + 2 * n].view(2 * values.shape[0], *values.shape[1:])
    view = doubled.chunk(2)[1]
    view.copy_(values)
    return view


def sliced(values, filler=NAN):
    "`big[..., ::2]` over a base twice as wide: non-dense strides"
    n = values.numel()
    base = _flat(PAD + 2 * n + PAD, values, filler)
    big = base[PAD : PAD + 2 * n].view(*values.shape[:-1], 2 * values.shape[-1])
    view = big[..., ::2]
    view.copy_(values)
    return view


def permuted_other(values, filler=NAN):
    "storage in (N, H, C, W) order, permuted to NCHW: neither contiguous nor channels-last"
    n, c, h, w = values.shape
    base = _flat(PAD + values.numel() + PAD, values, filler)
    view = base[PAD : PAD + values.numel()].view(n, h, c, w).permute(0, 2, 1, 3)
    view.copy_(values)
    assert not view.is_contiguous() and not view.is_contiguous(memory_format=torch.channels_last)
    return view


def channels_last(values, filler=NAN):
    "dense channels-last storage (what `contiguous(memory_format=torch.channels_last)` makes), aligned: the in-place route (control)"
    base = _flat(PAD + values.numel() + PAD, values, filler)
    view = base.as_strided(tuple(values.shape), _channels_last_strides(values.shape), PAD)
    view.copy_(values)
    return view


def channels_last_offset(values, filler=NAN):
    "a channels-last base with one extra leading sample, `[1:]`: dense layout + offset (misaligned when a sample's byte count is odd in 16-byte units)"
    n, c, h, w = values.shape
    per = c * h * w
    base = _flat(PAD + per + values.numel() + PAD, values, filler)
    big = base.as_strided((n + 1, c, h, w), _channels_last_strides((n + 1, c, h, w)), PAD)
    view = big[1:]
    view.copy_(values)
    return view


def expanded(values, filler=NAN):
    "one sample `expand`ed over the batch (stride 0): the storage is smaller than numel.  `values` must repeat its first sample"
    per = values[:1].numel()
    assert torch.equal(values.view(INT_VIEW[values.dtype]), values[:1].expand_as(values).contiguous().view(INT_VIEW[values.dtype])), "expanded: batch-constant values only"
    base = _flat(PAD + per + PAD, values, filler)
    one = base[PAD : PAD + per].view(1, *values.shape[1:])
    one.copy_(values[:1])
    return one.expand(values.shape)


KINDS = {
    "offset_small": offset_small, "offset_8": offset_8, "chunk_second": chunk_second, "sliced": sliced, "permuted_other": permuted_other,
    "channels_last": channels_last, "channels_last_offset": channels_last_offset, "expanded": expanded,
}  # fmt: skip


def same_tensor(values, filler=NAN):
    "ONE tensor for two operand roles (`model_output is sample`, `uncond is cond`): role tables keyed by id()"
    view = plain(values, filler)
    return view, view


def overlapping(values, filler=NAN):
    "two windows of one base shifted by 8 elements: the second operand's numbers are the first's, 8 further on (its last 8 are the first 8 again)"
    n = values.numel()
    base = _flat(PAD + n + 8 + PAD, values, filler)
    flat = values.reshape(-1)
    base[PAD : PAD + n].copy_(flat)
    base[PAD + n : PAD + n + 8].copy_(flat[:8])
    return base[PAD : PAD + n].view(values.shape), base[PAD + 8 : PAD + 8 + n].view(values.shape)


PAIR_KINDS = {"same_tensor": same_tensor, "overlapping": overlapping}
# the required mixed cases: (kind of the sample, kind of the model output)
MIXED = {
    "sample_channels_last+output_contiguous": ("channels_last", None),
    "sample_contiguous+output_channels_last": (None, "channels_last"),
    "sample_offset_8+output_sliced": ("offset_8", "sliced"),
}
ALL_KINDS = [*KINDS, *PAIR_KINDS, *MIXED]

# Entries that REFUSE a view instead of normalising it (clause 2).  Nothing of entries 1-8 may stand here: those normalise.
# name -> (exception type, what the message must name)
REFUSES = {
    "RollingBatch.step/sliced model_output": (ValueError, "model output"),
    "RollingBatch.step_guided/sliced uncond": (ValueError, "uncond"),
    "RollingBatch.step_guided/sliced cond": (ValueError, "cond"),
}
# capture_sampling_loop is NOT listed: it documents no refusal (`example` "fixes shape/dtype/device") and clones the example into its
# static buffer, so a non-contiguous example is normalised -- checked under clause (1) by the GPU module.


# ---- what the clauses look at ----------------------------------------------------------------------------------------------------
def twin(view: torch.Tensor) -> torch.Tensor:
    "a fresh, contiguous, 16-byte-aligned clone of the same values"
    c = view.detach().clone(memory_format=torch.contiguous_format)
    assert c.is_contiguous() and c.data_ptr() % 16 == 0
    return c


def bits(t) -> torch.Tensor:
    "the logical elements of `t` as integers of its storage dtype"
    t = concrete(t)
    return t.detach().contiguous().view(INT_VIEW[t.dtype])


def concrete(v) -> torch.Tensor:
    "a result as a tensor (a lazily evaluated prediction is materialised; an ndarray is wrapped)"
    if hasattr(v, "materialize"):
        v = v.materialize()
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(v)


def same_bits(a, b) -> bool:
    a, b = concrete(a), concrete(b)
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.device == b.device and torch.equal(bits(a), bits(b))


def storage_bytes(t: torch.Tensor) -> torch.Tensor:
    "every byte of the allocation behind `t`, padding included"
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def is_dense_channels_last(t: torch.Tensor) -> bool:
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def is_callers(got, operands) -> bool:
    """`got` is one of the caller's own tensors handed back, itself or through a view object of the same extent: what a record's `sample`
    / `prediction` fields and pred_original_sample are when the step leaves the model output as it is (reference structured.py: the
    record holds its inputs)"""
    got = got if isinstance(got, torch.Tensor) else None
    return got is not None and any(got is t or (got.data_ptr() == t.data_ptr() and got.shape == t.shape and got.stride() == t.stride()) for t in operands if isinstance(t, torch.Tensor))


def sync(device) -> None:
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


class Watch:
    "clauses (3) and (4) for one call: snapshots of the operands' whole bases, and their address ranges"

    def __init__(self, *operands):
        self.held = []
        seen = set()
        for t in operands:
            if isinstance(t, torch.Tensor) and t.untyped_storage().data_ptr() not in seen:
                seen.add(t.untyped_storage().data_ptr())
                raw = storage_bytes(t.detach())
                self.held.append((raw, raw.clone()))
        self.all_channels_last = all(is_dense_channels_last(t) for t in operands if isinstance(t, torch.Tensor))

    def assert_untouched(self, what: str) -> None:
        for raw, before in self.held:
            sync(raw.device)
            assert torch.equal(raw, before), f"{what}: the caller's storage changed (clause 3)"

    def assert_engine_owned(self, out, what: str, must_be_channels_last: bool = False, copy_of=None) -> None:
        """`copy_of`: the operand `out` may be the engine's snapshot of (a wrapper that does not alias its history hands the model output
        back as its own copy, in the caller's channels-last layout when it has one): such a copy is held to the overlap clause and to
        being contiguous or dense channels-last, not to the layout of the OTHER operands"""
        out = concrete(out)
        if copy_of is not None and same_bits(out, copy_of) and is_dense_channels_last(out) and is_dense_channels_last(copy_of):
            lo = out.untyped_storage().data_ptr()
            assert all(lo + out.untyped_storage().nbytes() <= raw.data_ptr() or raw.data_ptr() + raw.numel() <= lo for raw, _ in self.held), f"{what}: a result overlaps an operand's base (clause 4)"
            return
        lo = out.untyped_storage().data_ptr()
        hi = lo + out.untyped_storage().nbytes()
        for raw, _ in self.held:
            a = raw.data_ptr()
            assert hi <= a or a + raw.numel() <= lo, f"{what}: a result overlaps an operand's base (clause 4)"
        assert out.is_contiguous() or is_dense_channels_last(out), f"{what}: a result is neither contiguous nor dense channels-last: strides {out.stride()}"
        if not self.all_channels_last:
            assert out.is_contiguous(), f"{what}: some operand of the call is not channels-last, the result must be contiguous (clause 4)"
        if must_be_channels_last:
            assert is_dense_channels_last(out), f"{what}: every operand of the step shares one dense channels-last layout, the result must too (clause 4)"


def byte_sizes(operands) -> list:
    "the distinct byte sizes of the operands' allocations (what the churn allocates, once the operands themselves are dropped)"
    return sorted({t.untyped_storage().nbytes() for t in operands if isinstance(t, torch.Tensor)} | {t.numel() * t.element_size() for t in operands if isinstance(t, torch.Tensor)})


def churn(sizes, device) -> None:
    """Stale-pointer churn, BEST EFFORT.  The caller has DROPPED its references to the previous call's operands (the wrapper keeps alive
    what its history still reads); then eight NaN tensors of exactly each of the operands' byte sizes are allocated, synchronised and
    freed, so that a block the engine's temporaries or the caller's dropped operands gave back to the allocator has most likely been
    handed out and overwritten before the next step -- a remembered pointer that outlived its tensor then reads NaN.  It relies on the
    caching allocator reusing freed blocks of the same size, which is likely and not guaranteed."""
    junk = [torch.full((size,), 0xFF, dtype=torch.uint8, device=device) for size in sizes if size for _ in range(8)]  # (all-ones bytes: NaN in every float type)
    sync(device)
    del junk


def values(shape, dtype, device, seed: int, scale: float = 1.0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype).to(device)


def build(kind, vals: dict, filler=NAN) -> dict:
    """operands of one call: `kind` is None (every role a fresh contiguous tensor), the name of a single kind (every role that kind;
    `expanded`: the batch-constant roles only), the name of a pair kind (the first two roles), a MIXED name or a {role: kind} dict.
    Returns {role: tensor}; a pair kind REPLACES the second role's numbers (they are the first role's, same or shifted)."""
    roles = list(vals)
    if kind is None:
        return {r: twin(v) for r, v in vals.items()}
    if isinstance(kind, str) and kind in PAIR_KINDS:
        a, b = PAIR_KINDS[kind](vals[roles[0]], filler)
        return {roles[0]: a, roles[1]: b, **{r: twin(vals[r]) for r in roles[2:]}}
    if isinstance(kind, str) and kind in MIXED:
        kind = dict(zip(roles, MIXED[kind]))
    if isinstance(kind, str):
        kind = {r: kind for r in roles}
    # (an `expanded` operand holds its first sample over the whole batch: the role's numbers become that)
    return {r: (KINDS[kind[r]](batch_constant(v) if kind[r] == "expanded" else v, filler) if kind.get(r) else twin(v)) for r, v in vals.items()}


def batch_constant(v: torch.Tensor) -> torch.Tensor:
    "the values an `expanded` operand can hold: the first sample repeated"
    return v[:1].expand_as(v).contiguous()


# ---- wrapper runs: two wrappers in lockstep, one fed views, one fed fresh contiguous clones ---------------------------------------
def plan_of(schedule: str, kind, steps: int) -> list:
    "which steps of a run get views: (a) all of them, (b) steps 2 and 4 (run 2, after a contiguous run 1), (c) alternating from step 0"
    if schedule == "a":
        return [kind] * steps
    if schedule == "b":
        return [kind if i in (2, 4) else None for i in range(steps)]
    if schedule == "c":
        return [kind if i % 2 == 0 else None for i in range(steps)]
    raise KeyError(schedule)


def seeds_for(device, batch: int):
    "per-sample noise seeds as the wrappers take them: ints on the HIP device (Philox keys), torch generators on the host"
    return [11 + b for b in range(batch)] if torch.device(device).type == "cuda" else [torch.Generator().manual_seed(11 + b) for b in range(batch)]


def run_pair(make, shape, dtype, device, plan: list, seed: int, *, guided=None, rescale: float = 0.0, inpaint=None, oracle=None, warm_run: bool = False,
             exact=None, run_steps: int | None = None, label: str = "") -> dict:  # fmt: skip
    """One run of len(plan) steps on two wrappers from `make()`: `wv` gets the operands plan[i] describes, `wc` fresh contiguous clones
    of the same numbers.  After every call: clause (1) on prev_sample and pred_original_sample, clause (3) on every operand's base,
    clause (4) on both results; then the churn, for both runs alike.  The next sample is the view run's own prev_sample (bit-equal to
    the other's by then).
    guided: None, or a function step index -> guidance scale or None (None: a plain step() in a guided run); the roles are then
        (uncond, cond, sample).  Without a rescale (whose statistic is the device's own launch) the contiguous run is also held, bit for
        bit, to a third wrapper that gets step() on torch's own three lines; the 16-bit fp16 case is the `exact` rule below instead.
    inpaint: None, or (mask kind, original kind, noise kind): set_inpaint on both wrappers before the first step.
    oracle: None, or a function (i, t, operands of the contiguous run, result) that holds the contiguous run to the family's oracle.
    warm_run: schedule (b) -- a first run on contiguous tensors, so that step programs and replayed entries exist; returns the replay
        counters of run 2.
    exact: fp16 guided cases: a function (i, t, contiguous operands) -> float64 (prev_sample, pred_original_sample); clause
        (1) on both is then the suite's no_further_from_exact rule, both distances recorded."""
    steps = len(plan)
    wv, wc = make(), make()
    outs = [values(shape, dtype, device, seed * 100 + i) for i in range(2 * steps)]
    x0 = values(shape, dtype, device, seed * 100 + 99)
    notes = {"hits_view": 0, "hits_contiguous": 0, "margins": [], "bindable": []}
    if warm_run:
        for w in (wv, wc):
            w.set_timesteps(run_steps or steps)
            x, sd = twin(x0), seeds_for(device, shape[0])
            for i, t in enumerate(w.timesteps.tolist()):
                # (warm_run == "views": the view wrapper meets its views in run 1 already -- whatever it learns there must not be replayed wrongly in run 2)
                ops = build(plan[i] if warm_run == "views" and w is wv else None, {"sample": x, "model_output": outs[i]})
                x = concrete(w.step(ops["model_output"], t, ops["sample"], generator=sd, return_dict=False)[0])
        sync(device)
    for w in (wv, wc):
        w.set_timesteps(run_steps or steps)  # (`run_steps`: a Runge-Kutta wrapper is called once per STAGE -- len(plan) calls of a shorter schedule)
    if inpaint is not None:
        mk, ok, nk = inpaint
        mvals = batch_constant((values((shape[0], 1, *shape[2:]), dtype, device, seed * 100 + 97) > 0).to(dtype))
        ivals = {"original_samples": values(shape, dtype, device, seed * 100 + 96), "noise": values(shape, dtype, device, seed * 100 + 95)}
        mask_v = KINDS[mk](mvals) if mk else twin(mvals)
        iv = {r: (KINDS[k](ivals[r]) if k else twin(ivals[r])) for r, k in zip(ivals, (ok, nk))}
        inpaint_watch = Watch(mask_v, *iv.values())
        wv.set_inpaint(mask_v, iv["original_samples"], iv["noise"])
        wc.set_inpaint(twin(mvals), twin(ivals["original_samples"]), twin(ivals["noise"]))
    hits0 = (getattr(wv, "_fast_hits", 0), getattr(wc, "_fast_hits", 0))
    sv, sc, st = (seeds_for(device, shape[0]) for _ in range(3))
    wt = None
    if guided is not None and exact is None and rescale == 0.0 and inpaint is None:
        wt = make()
        wt.set_timesteps(run_steps or steps)
    x = x0
    run_all_channels_last = True
    times = wv.timesteps.tolist()[:steps]
    assert len(times) == steps, (len(times), steps)
    for i, t in enumerate(times):
        scale = guided(i) if guided is not None else None
        if scale is not None:
            vals = {"uncond": outs[i], "cond": outs[steps + i], "sample": x}
        else:
            vals = {"sample": x, "model_output": outs[i]}
        kind = plan[i]
        ops_v = build(kind, vals)
        ops_c = {r: twin(v) for r, v in ops_v.items()}
        watch = Watch(*ops_v.values())
        notes["bindable"].append(all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in ops_v.values()))
        run_all_channels_last = run_all_channels_last and watch.all_channels_last and (inpaint is None or all(is_dense_channels_last(t) for t in iv.values()))
        what = f"{label} step {i} kind {kind}"
        if scale is not None:
            rv = wv.step_guided(ops_v["uncond"], ops_v["cond"], scale, t, ops_v["sample"], generator=sv, return_dict=False, guidance_rescale=rescale)
            rc = wc.step_guided(ops_c["uncond"], ops_c["cond"], scale, t, ops_c["sample"], generator=sc, return_dict=False, guidance_rescale=rescale)
        else:
            rv = wv.step(ops_v["model_output"], t, ops_v["sample"], generator=sv, return_dict=False)
            rc = wc.step(ops_c["model_output"], t, ops_c["sample"], generator=sc, return_dict=False)
        prev_v, pred_v, prev_c, pred_c = concrete(rv[0]), concrete(rv[1]), concrete(rc[0]), concrete(rc[1])
        ops_t = rt = None
        if wt is not None:  # the contiguous guided run against step() on torch's own three lines (README: "the bits of step(uncond + g * (cond - uncond), ...)")
            ops_t = {r: twin(v) for r, v in ops_v.items()}
            lines = ops_t["uncond"] + scale * (ops_t["cond"] - ops_t["uncond"]) if scale is not None else ops_t["model_output"]
            rt = wt.step(lines, t, ops_t["sample"], generator=st, return_dict=False)
            assert same_bits(prev_c, rt[0]) and same_bits(pred_c, rt[1]), f"{what}: the contiguous guided run differs from step() on torch's three lines"
        sync(device)
        if exact is not None and scale is not None:
            from conftest import note_margin
            from test_noise_gpu import no_further_from_exact

            for field, got_v, got_c, e in zip(("prev_sample", "pred_original_sample"), (prev_v, pred_v), (prev_c, pred_c), exact(i, t, ops_c)):
                dist = lambda g: ((g.detach().cpu().double() - e).abs().max() / e.abs().max()).item()  # noqa: E731, B023
                notes["margins"].append((note_margin("operand views fp16 guided", f"{label} {field}: view run vs float64", dist(got_v), None),
                                         note_margin("operand views fp16 guided", f"{label} {field}: contiguous run vs float64", dist(got_c), None)))
                assert no_further_from_exact(got_v, got_c, e), (what, field, notes["margins"][-1])
        else:
            assert same_bits(prev_v, prev_c), f"{what}: prev_sample differs from the contiguous run (clause 1)"
            assert same_bits(pred_v, pred_c), f"{what}: pred_original_sample differs from the contiguous run (clause 1)"
        watch.assert_untouched(what)
        if inpaint is not None:
            inpaint_watch.assert_untouched(what + " (in-paint tensors)")
        # "exactly when": the step kernels' in-place route (README "channels-last latents").  Not asked of the routes DESIGN.md lists as out
        # of its scope, which copy and return contiguous results: the op tape (compute_scale=None on 16-bit tensors), the Runge-Kutta
        # stages, and a draw that is realised to a (contiguous) tensor, which makes the launch a mixed one
        strict = run_all_channels_last and getattr(wv, "compute_scale", None) is not None and hasattr(wv, "sampler") and not wv.sampler.require_noise
        watch.assert_engine_owned(prev_v, what + " prev_sample", must_be_channels_last=strict)
        if not is_callers(pred_v, ops_v.values()):  # (a stated sampler's pred_original_sample IS the caller's model output)
            watch.assert_engine_owned(pred_v, what + " pred_original_sample", copy_of=ops_v.get("model_output"))
        if oracle is not None:
            oracle(i, t, ops_c, prev_c)
        x = prev_v if exact is None else prev_c
        sizes = byte_sizes([*ops_v.values(), *ops_c.values()])
        del ops_v, ops_c, ops_t, watch, rv, rc, rt, vals, prev_v, pred_v, prev_c, pred_c  # every reference of the caller's but the next sample
        churn(sizes, device)
    notes["hits_view"], notes["hits_contiguous"] = getattr(wv, "_fast_hits", 0) - hits0[0], getattr(wc, "_fast_hits", 0) - hits0[1]
    return notes


def reused_buffer_pair(make, shape, dtype, device, kind: str, seed: int, steps: int = 6) -> None:
    """The static-buffer caller: `sample` and `model_output` are views of two PERSISTENT bases that the caller refills in place before every
    step (a graphed network's output memory, an in-place `buf.copy_()` loop).  With the default alias_history="auto" the wrapper's documented
    behaviour is to notice this on the run's second call and to snapshot from then on, so the whole run has the bits of the contiguous
    run; a wrapper that kept aliasing such operands would read refilled history -- or trip its guard ("was modified in place since")."""
    wv, wc = make(), make()
    for w in (wv, wc):
        w.set_timesteps(steps)
    x = values(shape, dtype, device, seed * 100 + 99)
    buf_x, buf_o = KINDS[kind](torch.zeros_like(x)), KINDS[kind](torch.zeros_like(x))
    sv, sc = seeds_for(device, shape[0]), seeds_for(device, shape[0])
    for i, t in enumerate(wv.timesteps.tolist()):
        buf_x.copy_(x)
        buf_o.copy_(values(shape, dtype, device, seed * 100 + i))
        watch = Watch(buf_x, buf_o)
        rv = wv.step(buf_o, t, buf_x, generator=sv, return_dict=False)
        rc = wc.step(twin(buf_o), t, twin(buf_x), generator=sc, return_dict=False)
        sync(device)
        what = f"reused buffers {kind} {tuple(shape)} {dtype} step {i}"
        assert same_bits(rv[0], rc[0]) and same_bits(rv[1], rc[1]), f"{what}: differs from the contiguous run (clause 1)"
        watch.assert_untouched(what)
        watch.assert_engine_owned(rv[0], what)
        x = concrete(rv[0]).clone()


def expected_replays(keep: int, bindable: list) -> tuple:
    """(view run, contiguous run): how many steps of run 2 of schedule (b) the wrapper serves from its replayed entries.  `bindable[i]`: step
    i's operands were contiguous and 16-byte aligned, which is what an entry learned on contiguous tensors binds (a `chunk` half at an
    even address, one tensor in two roles and overlapping windows are such operands; a slice, a permutation, channels-last storage and
    an odd address are not).  A sampler without history replays every bindable step; one with history settles its alias mode over the
    first two calls, and a replayed step binds its history by pointer, so it is only taken when every record of its window was
    bindable too."""
    first = 2 if keep else 0
    full = len(bindable) - first
    view = sum(1 for i in range(first, len(bindable)) if all(bindable[max(i - keep, 0) : i + 1]))
    return view, full


# ---- sampler.sample(...) called directly ---------------------------------------------------------------------------------------------
def sampler_pair(sampler, model, schedule, shape, dtype, device, kind, seed: int, *, steps: int = 4, noise: bool = False, roles=None, oracle=None, label: str = "") -> torch.Tensor:
    """`steps` calls of sampler.sample on views and, in lockstep, on fresh contiguous clones; the `previous` records of the view run are the
    records its own earlier calls returned (so their fields are, or were computed from, views).  `roles`: the roles that get the kind
    (default: all of sample, prediction, noise).  Clauses (1), (3), (4) after every call, on `final` and on every record field that
    is read (`sample`, `prediction`).  Returns the last result."""
    from skrample_amd.common import Step

    total = steps + 2
    prev_v, prev_c = [], []
    mk = (lambda s: batch_constant(values(shape, dtype, device, s))) if kind == "expanded" else (lambda s: values(shape, dtype, device, s))
    x = mk(seed * 100 + 99)
    all_cl = True
    for i in range(steps):
        vals = {"sample": x, "prediction": mk(seed * 100 + i)}
        if noise:
            vals["noise"] = mk(seed * 100 + 50 + i)
        spec = kind if roles is None or kind is None or kind in PAIR_KINDS or kind in MIXED else {r: kind for r in roles}
        ops_v = build(spec, vals)
        ops_c = {r: twin(v) for r, v in ops_v.items()}
        watch = Watch(*ops_v.values())
        all_cl = all_cl and watch.all_channels_last
        what = f"{label} {type(sampler).__name__} {tuple(shape)} {dtype} step {i} kind {spec}"
        step = Step.from_int(i, total)
        rv = sampler.sample(ops_v["sample"], ops_v["prediction"], step, model, schedule, ops_v.get("noise"), tuple(prev_v))
        rc = sampler.sample(ops_c["sample"], ops_c["prediction"], step, model, schedule, ops_c.get("noise"), tuple(prev_c))
        sync(device)
        for field in ("final", "sample", "prediction"):
            assert same_bits(getattr(rv, field), getattr(rc, field)), f"{what}: record field `{field}` differs from the contiguous run (clause 1)"
        watch.assert_untouched(what)
        final = concrete(rv.final)
        watch.assert_engine_owned(final, what + " final", must_be_channels_last=all_cl and dtype in (torch.float32, torch.float64))
        for field in ("sample", "prediction"):
            got = getattr(rv, field)
            if not is_callers(got, ops_v.values()):  # (a stated sampler's record names the caller's own tensors)
                watch.assert_engine_owned(got, what + " " + field)
        if oracle is not None:
            oracle(i, step, ops_c, rc)
        keep = max(sampler.require_previous, 1)
        prev_v, prev_c = [*prev_v, rv][-keep:], [*prev_c, rc][-keep:]
        x = final
        del ops_v, ops_c, watch
    return x


# ---- autograd: gradients reach the BASE of a view ------------------------------------------------------------------------------------
def grad_view(view: torch.Tensor):
    "(base, view): the whole allocation behind `view` as a leaf that requires grad, and the same view taken from it by a recorded op"
    base = torch.empty(0, dtype=view.dtype, device=view.device).set_(view.untyped_storage()).requires_grad_(True)
    return base, base.as_strided(tuple(view.shape), view.stride(), view.storage_offset())


def scattered(base: torch.Tensor, view: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
    "what base.grad must be: `grad` at the view's positions, zero elsewhere"
    want = torch.zeros_like(base)
    want.as_strided(tuple(view.shape), view.stride(), view.storage_offset()).copy_(grad)
    return want
