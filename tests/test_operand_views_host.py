"""Operand views on host-resident operands (CPU tensors, numpy arrays) through the package's host executor: the matrix of
tests/view_cases.py -- clauses (1) same bits as the contiguous run, (3) the caller's storage untouched, (4) results the engine's own --
for sampler.sample called directly, whole wrapper runs (schedules a and c), step_guided, the noise / model transforms on 16-bit tensors
and autograd.  The device half, with the replay guards, in-painting, Runge-Kutta stages, generators and the refusing entries, is
tests/test_operand_views_gpu.py."""

import numpy as np
import pytest
import torch
import view_cases as VC
from test_step_gpu import assert_close

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skr_oracle import samplers as OA
from skr_oracle import schedules as OS
from skr_oracle import wrapper as OW
from skrample_amd.common import Point, Step
from skrample_amd.sampling import models as PM
from skrample_amd.sampling import structured as PT

CPU = torch.device("cpu")

WRAPPERS = {
    # name: (wrapper factory, oracle sampler config, oracle schedule)
    "euler": (lambda **kw: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled(), **kw), lambda: OA.make("euler"), OS.scaled),
    "dpm3_sde": (lambda **kw: PD.SkrampleWrapperScheduler(PT.DPM(order=3, stochasticity=1), PS.Scaled(), **kw), lambda: OA.make("dpm", 3, eta=1), OS.scaled),
    "adams4": (lambda **kw: PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.Scaled(), **kw), lambda: OA.make("adams", 4), OS.scaled),
    "unipc3": (lambda **kw: PD.SkrampleWrapperScheduler(PT.UniPC(order=3), PS.Scaled(), **kw), lambda: OA.make("unipc", 3), OS.scaled),
    "spc": (lambda **kw: PD.SkrampleWrapperScheduler(PT.SPC(), PS.Scaled(), **kw), lambda: OA.make("spc"), OS.scaled),
}
STEPS = 6
# (latent dtype, compute_scale); None on 16-bit latents is the op tape
CONFIGS = ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.bfloat16, None), (torch.float16, None))


def step_oracle(name, dtype):
    "the contiguous run against the oracle's step driver, at test_step_gpu.assert_close (deterministic samplers: the oracle needs no draw)"
    _mk, cfg, sched = WRAPPERS[name]
    driver = OW.StepDriver(cfg(), sched(), "eps")
    driver.set_timesteps(STEPS)

    def check(i, t, ops, got):
        ref = driver.step(ops["model_output"].cpu(), t, ops["sample"].cpu())[0]
        assert_close(got, ref, dtype, f"{name} contiguous run vs oracle, step {i}")

    return check


# ---- entry 1: sampler.sample called directly ----------------------------------------------------------------------------------------------
def euler_oracle(i, step, ops, rec):
    ref = OA.sample(OA.make("euler", eta=1), ops["sample"], ops["prediction"], tuple(step), "eps", OS.scaled(), ops["noise"]).final
    assert_close(rec.final, ref, ops["sample"].dtype, f"Euler contiguous run vs OA.sample, step {i}")


@pytest.mark.parametrize("kind", VC.ALL_KINDS)
def test_sampler_sample_euler_with_a_noise_tensor(kind):
    "three operands to vary: each of sample, prediction, noise alone as the view, then all three (fp32: the fused form; bf16 / fp16: the op tape)"
    smp = PT.Euler(stochasticity=1)
    for shape in VC.SHAPES[:2]:
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            subsets = [None] if kind in VC.PAIR_KINDS or kind in VC.MIXED else [("sample",), ("prediction",), ("noise",), None]
            for roles in subsets:
                VC.sampler_pair(smp, PM.NoiseModel(), PS.Scaled(), shape, dtype, CPU, kind, 1, steps=2, noise=True, roles=roles,
                                oracle=euler_oracle if dtype == torch.float32 and roles is None else None)


@pytest.mark.parametrize("kind", VC.ALL_KINDS)
@pytest.mark.parametrize("name", ["dpm2", "adams3", "unipc2"])
def test_sampler_sample_multistep_with_records_made_from_views(name, kind):
    smp = {"dpm2": PT.DPM(order=2), "adams3": PT.Adams(order=3), "unipc2": PT.UniPC(order=2)}[name]
    for shape in VC.SHAPES[:2]:
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            VC.sampler_pair(smp, PM.NoiseModel(), PS.Scaled(), shape, dtype, CPU, kind, 2, steps=4)


def test_sampler_sample_float64():
    for kind in ("sliced", "offset_small", "channels_last_offset"):
        VC.sampler_pair(PT.DPM(order=2), PM.VelocityModel(), PS.ZSNR(), (2, 4, 5, 7), torch.float64, CPU, kind, 3, steps=3)


def test_chunk_second_of_a_280_byte_sample():
    "the `uncond, cond = noise_pred.chunk(2)` idiom at (1, 4, 5, 7): a bf16 half is 280 bytes, the second half sits 8 bytes past a 16-byte line"
    v = VC.chunk_second(VC.values(VC.CHUNK_SHAPE, torch.bfloat16, CPU, 0))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    for dtype in (torch.bfloat16, torch.float32):
        VC.sampler_pair(PT.DPM(order=2), PM.NoiseModel(), PS.Scaled(), VC.CHUNK_SHAPE, dtype, CPU, "chunk_second", 4, steps=3)


# ---- entry 2: whole wrapper runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["a", "c"])
@pytest.mark.parametrize("kind", VC.ALL_KINDS)
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_runs(name, kind, schedule):
    mk = WRAPPERS[name][0]
    for shape in VC.SHAPES[:2]:
        for dtype, scale in CONFIGS:
            oracle = step_oracle(name, dtype) if name != "dpm3_sde" and scale is not None and kind == "sliced" and schedule == "a" else None
            VC.run_pair(lambda: mk(compute_scale=scale), shape, dtype, CPU, VC.plan_of(schedule, kind, STEPS), 5, oracle=oracle, label=f"{name}/{scale}/{schedule}")
        # invert_prediction without a compute scale: the negated prediction is a tape expression of its own in front of the step
        VC.run_pair(lambda: mk(compute_scale=None, invert_prediction=True), shape, torch.bfloat16, CPU, VC.plan_of(schedule, kind, STEPS), 5, label=f"{name}/inverted/{schedule}")


def check_rk(device, kind, shapes):
    "RKUltraWrapperScheduler with a three-stage tableau, one call per stage: the second stage of every step gets the views"
    for scale, dtypes in ((torch.float32, (torch.bfloat16, torch.float32)), (None, (torch.bfloat16, torch.float16))):  # (None on 16-bit tensors: the op tape)
        mk = lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=3, stochasticity=0.5, compute_scale=scale)  # noqa: E731, B023
        probe = mk()
        probe.set_timesteps(3)
        calls, order = len(probe.timesteps), probe.order
        assert order == 3
        plan = [kind if i % order == 1 else None for i in range(calls)]
        for shape in shapes:
            for dtype in dtypes:
                VC.run_pair(mk, shape, dtype, device, plan, 11, run_steps=3, label=f"rku3/{scale}")


@pytest.mark.parametrize("kind", VC.ALL_KINDS)
def test_rk_wrapper_views_at_stage_two(kind):
    check_rk(CPU, kind, VC.SHAPES[:2])


@pytest.mark.parametrize("kind", ["sliced", "offset_8", "channels_last"])
@pytest.mark.parametrize("name", ["dpm3_sde", "adams4", "unipc3"])
def test_wrapper_run_on_views_of_buffers_refilled_in_place(name, kind):
    for dtype in (torch.float32, torch.bfloat16):
        VC.reused_buffer_pair(WRAPPERS[name][0], VC.SHAPES[0], dtype, CPU, kind, 15)


# ---- entry 3: step_guided ----------------------------------------------------------------------------------------------------------------
GUIDED_KINDS = {
    "chunk_second": {"uncond": "chunk_second", "cond": "chunk_second"},
    "uncond_plain+cond_chunk_second": {"cond": "chunk_second"},
    "offset_8": {"uncond": "offset_8", "cond": "offset_8"},
    "same_tensor": "same_tensor",
    "sliced": {"uncond": "sliced", "cond": "sliced", "sample": "sliced"},
    "cond_channels_last": {"cond": "channels_last"},
    "uncond_channels_last": {"uncond": "channels_last"},
    "overlapping": "overlapping",
    "expanded_cond": {"cond": "expanded"},
}


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("kind", GUIDED_KINDS)
@pytest.mark.parametrize("name", ["euler", "dpm3_sde", "unipc3"])
def test_step_guided(name, kind, rescale):
    "guided calls on views, mixed with plain step() calls in one run (steps 1 and 4 are plain)"
    mk = WRAPPERS[name][0]
    spec = GUIDED_KINDS[kind]
    for shape in (VC.CHUNK_SHAPE, VC.SHAPES[1]):
        for dtype in (torch.bfloat16, torch.float32):
            plan = [spec if i not in (1, 4) else "sliced" for i in range(STEPS)]
            VC.run_pair(mk, shape, dtype, CPU, plan, 6, guided=lambda i: None if i in (1, 4) else 5.5, rescale=rescale, label=f"guided {name}/{kind}")


# ---- entry 6: add_noise / scale_noise / remove_noise, to_x / from_x on 16-bit tensors (tape entries) ------------------------------------
def transform_cases(device):
    point = Point(500.0, 0.7, 0.6)
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled())
    w.set_timesteps(STEPS)
    t = w.timesteps[2:3]
    return {
        "Point.add_noise": lambda a, b: point.add_noise(a, b),
        "Point.remove_noise": lambda a, b: point.remove_noise(a, b),
        "wrapper.add_noise": lambda a, b: w.add_noise(a, b, t),
        "wrapper.scale_noise": lambda a, b: w.scale_noise(a, t[0], b),
        "NoiseModel.to_x": lambda a, b: PM.NoiseModel().to_x(a, b, point),
        "VelocityModel.from_x": lambda a, b: PM.VelocityModel().from_x(a, b, point),
        "FlowModel.to_x": lambda a, b: PM.FlowModel().to_x(a, b, point),
    }


def check_transforms(device, kind, dtypes):
    for shape in VC.SHAPES[:2]:
        for dtype in dtypes:
            vals = {"a": VC.values(shape, dtype, device, 7), "b": VC.values(shape, dtype, device, 8)}
            if kind == "expanded":
                vals = {r: VC.batch_constant(v) for r, v in vals.items()}
            for name, fn in transform_cases(device).items():
                ops = VC.build(kind, vals)
                twins = {r: VC.twin(v) for r, v in ops.items()}
                watch = VC.Watch(*ops.values())
                got, ref = fn(ops["a"], ops["b"]), fn(twins["a"], twins["b"])
                what = f"{name} {shape} {dtype} kind {kind}"
                assert VC.same_bits(got, ref), f"{what}: differs from the contiguous call (clause 1)"
                watch.assert_untouched(what)
                watch.assert_engine_owned(got, what)


@pytest.mark.parametrize("kind", VC.ALL_KINDS)
def test_noise_and_model_transforms(kind):
    check_transforms(CPU, kind, (torch.bfloat16, torch.float16, torch.float32))


# ---- entry 8: autograd --------------------------------------------------------------------------------------------------------------------
def check_autograd(device, kind, dtype, inpaint=False):
    "two DPM-2 wrapper steps on views of bases that require grad; the second step's result is differentiated: base.grad = the contiguous run's grad scattered"
    shape = VC.SHAPES[0]
    runs = []
    for views in (True, False):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled())
        w.set_timesteps(STEPS)
        if inpaint:
            mask = (VC.values((shape[0], 1, *shape[2:]), dtype, device, 40) > 0).to(dtype)
            w.set_inpaint(mask, VC.values(shape, dtype, device, 41), VC.values(shape, dtype, device, 42))
        leaves, x = [], None
        for i, t in enumerate(w.timesteps.tolist()[:2]):
            pair = []
            for role, seed in (("model_output", 30 + i), ("sample", 35)):
                v = VC.values(shape, dtype, device, seed)
                if role == "sample" and i > 0:
                    pair.append(x)
                    continue
                if views:
                    view = VC.KINDS[kind](v, 0.5)
                    base, gv = VC.grad_view(view)
                    leaves.append((base, view))
                    pair.append(gv)
                else:
                    c = VC.twin(v).requires_grad_(True)
                    leaves.append((c, None))
                    pair.append(c)
            x = VC.concrete(w.step(pair[0], t, pair[1], return_dict=False)[0])
        weight = VC.values(shape, torch.float32, device, 50)
        (x.float() * weight).sum().backward()
        VC.sync(device)
        runs.append((x.detach(), leaves))
    (xv, lv), (xc, lc) = runs
    assert VC.same_bits(xv, xc), f"autograd {kind} {dtype}: the recorded forward differs from the contiguous run (clause 1)"
    for k, ((base, view), (c, _)) in enumerate(zip(lv, lc)):
        assert c.grad is not None and base.grad is not None, k
        assert VC.same_bits(base.grad, VC.scattered(base, view, c.grad)), f"autograd {kind} {dtype}: leaf {k}: base.grad is not the contiguous run's grad scattered to the view's positions"
    return [c.grad for c, _ in lc]


@pytest.mark.parametrize("kind", ["sliced", "offset_small"])
def test_autograd_through_a_wrapper_step(kind):
    for dtype in (torch.float32, torch.bfloat16):
        check_autograd(CPU, kind, dtype)


# ---- numpy arrays ------------------------------------------------------------------------------------------------------------------------
def numpy_views(arr: np.ndarray) -> dict:
    "views with `arr`'s numbers into larger bases; name -> (view, base)"
    out = {}
    big = np.full(arr.shape[:-1] + (2 * arr.shape[-1],), np.nan, dtype=arr.dtype)
    big[..., ::2] = arr
    out["sliced"] = (big[..., ::2], big)
    flat = np.full(arr.size + 2 * VC.PAD + 1, np.nan, dtype=arr.dtype)
    window = flat[VC.PAD + 1 : VC.PAD + 1 + arr.size].reshape(arr.shape)
    window[...] = arr
    out["offset_small"] = (window, flat)
    rev = np.full(arr.size + 2 * VC.PAD, np.nan, dtype=arr.dtype)
    rev[VC.PAD : VC.PAD + arr.size] = arr.reshape(-1)[::-1]
    out["negative_stride"] = (rev[VC.PAD : VC.PAD + arr.size][::-1].reshape(arr.shape), rev)
    assert out["negative_stride"][0].strides[-1] < 0
    out["transposed"] = (np.ascontiguousarray(arr.T).T, None)
    return out


@pytest.mark.parametrize("kind", ["sliced", "offset_small", "negative_stride", "transposed"])
def test_numpy_array_views(kind):
    "ndarray views -- a negative-stride `arr[::-1]` among them, which torch.from_numpy refuses -- give the contiguous arrays' numbers and stay untouched"
    rng = np.random.default_rng(9)
    for dt in (np.float64, np.float32):
        for sampler in (PT.DPM(order=2), PT.UniPC(order=2)):
            prev_v, prev_c = [], []
            x = rng.standard_normal((3, 8)).astype(dt)
            for i in range(3):
                out = rng.standard_normal((3, 8)).astype(dt)
                (xv, xb), (ov, ob) = numpy_views(x)[kind], numpy_views(out)[kind]
                keep = [b.copy() for b in (xb, ob) if b is not None]
                rv = sampler.sample(xv, ov, Step.from_int(i, 6), PM.NoiseModel(), PS.Scaled(), None, tuple(prev_v))
                rc = sampler.sample(x.copy(), out.copy(), Step.from_int(i, 6), PM.NoiseModel(), PS.Scaled(), None, tuple(prev_c))
                assert isinstance(rv.final, np.ndarray) and rv.final.dtype == dt
                assert np.array_equal(rv.final.view(np.uint8), rc.final.view(np.uint8)), (kind, dt, sampler, i)
                for b, before in zip((b for b in (xb, ob) if b is not None), keep):
                    assert np.array_equal(b.view(np.uint8), before.view(np.uint8)), "the caller's array changed"
                assert not any(np.shares_memory(rv.final, b) for b in (xv, ov))
                prev_v, prev_c = [*prev_v, rv][-2:], [*prev_c, rc][-2:]
                x = rc.final


def test_numpy_view_reused_in_place_between_calls():
    "a strided ndarray the caller refills between calls (one array object, new numbers): the second call reads the new numbers"
    rng = np.random.default_rng(10)
    sampler = PT.Euler()
    big = np.zeros((3, 16))
    view = big[:, ::2]
    x = rng.standard_normal((3, 8))
    for i in range(3):
        fresh = rng.standard_normal((3, 8))
        view[...] = fresh
        got = sampler.sample(x, view, Step.from_int(i, 6), PM.NoiseModel(), PS.Scaled()).final
        ref = sampler.sample(x.copy(), fresh.copy(), Step.from_int(i, 6), PM.NoiseModel(), PS.Scaled()).final
        assert np.array_equal(got, ref), f"call {i}: a strided ndarray's earlier contents were used"
        x = ref


# ---- the matrix itself -------------------------------------------------------------------------------------------------------------------
def test_every_kind_builds_what_it_says():
    for dtype in (torch.bfloat16, torch.float32, torch.float64):
        item = torch.empty(0, dtype=dtype).element_size()
        for shape in [*VC.SHAPES, VC.CHUNK_SHAPE]:
            v = VC.values(shape, dtype, CPU, 1)
            for name, fn in VC.KINDS.items():
                view = fn(VC.batch_constant(v) if name == "expanded" else v)
                assert tuple(view.shape) == tuple(shape) and view.dtype == dtype
                assert VC.same_bits(view, VC.batch_constant(v) if name == "expanded" else v), name
                raw = VC.storage_bytes(view)
                lo = view.data_ptr() - raw.data_ptr()
                assert lo >= VC.PAD * item, (name, "padding in front")
                last = lo + sum((s - 1) * st for s, st in zip(view.shape, view.stride())) * item + item
                assert raw.numel() - last >= VC.PAD * item, (name, "padding behind")
            assert VC.offset_small(v).data_ptr() % 16 == item % 16 and VC.offset_8(v).data_ptr() % 16 == 8
            assert VC.offset_small(v).is_contiguous() and VC.offset_8(v).is_contiguous() and VC.chunk_second(v).is_contiguous()
            assert not VC.sliced(v).is_contiguous() and (shape[0] == 1 or VC.expanded(VC.batch_constant(v)).stride(0) == 0)
            assert VC.is_dense_channels_last(VC.channels_last(v)) and VC.is_dense_channels_last(VC.channels_last_offset(v))
            assert VC.channels_last(v).data_ptr() % 16 == 0
            a, b = VC.overlapping(v)
            assert b.data_ptr() - a.data_ptr() == 8 * item and VC.same_bits(a, v)
    assert VC.channels_last_offset(VC.values(VC.SHAPES[0], torch.bfloat16, CPU, 1)).data_ptr() % 16 == 8  # (a 280-byte sample)


def test_refusals_are_capped():
    "only RollingBatch and capture cases may refuse a view: entries 1-8 normalise"
    assert VC.REFUSES and all(name.startswith(("RollingBatch.", "capture_sampling_loop")) for name in VC.REFUSES)
    assert all(issubclass(exc, Exception) and isinstance(names, str) and names for exc, names in VC.REFUSES.values())
