"""Operand views on the HIP device (needs an MI355X): every Python entry point against its contiguous run, over the matrix of
tests/view_cases.py -- (1) same bits as the contiguous run, (2) or a documented refusal that changes nothing, (3) the caller's storage
untouched, (4) results the engine's own.  What the host half (tests/test_operand_views_host.py) cannot reach is here: the alignment
clones, the replayed steps and their remembered history pointers (schedule b), in-painting, the Runge-Kutta stages, the generators on a
caller's tensor, the masked backward, and the entries that refuse.  Between the steps of every wrapper run the operands are dropped and
their allocations churned with NaN (view_cases.churn: best effort -- it relies on the caching allocator reusing freed blocks)."""

import pytest
import torch
import view_cases as VC
from conftest import note_margin
from test_operand_views_host import CONFIGS, GUIDED_KINDS, STEPS, WRAPPERS, check_autograd, check_rk, check_transforms, euler_oracle, step_oracle
from test_step_gpu import assert_close

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skr_oracle import noise as ON
from skr_oracle import samplers as OA
from skr_oracle import schedules as OS
from skr_oracle import wrapper as OW
from skrample_amd import _hip
from skrample_amd.pytorch import noise as PN
from skrample_amd.sampling import lazy, native
from skrample_amd.sampling import models as PM
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _library():
    _hip.load()


# ---- entry 1: sampler.sample called directly ----------------------------------------------------------------------------------------------
def tape_oracle(sampler, model, schedule, noise):
    "the 16-bit route's bar (DESIGN.md 10: the op tape has the host interpreter's bits): the contiguous device run against the same call on CPU tensors"
    history = []

    def check(i, step, ops, rec):
        before = native.launches
        host = sampler.sample(ops["sample"].cpu(), ops["prediction"].cpu(), step, model, schedule, ops["noise"].cpu() if noise else None, tuple(history))
        history.append(host)
        del history[: max(len(history) - max(sampler.require_previous, 1), 0)]
        assert native.launches == before, "the host twin must not launch"
        assert VC.same_bits(VC.concrete(rec.final).cpu(), host.final), f"tape route, step {i}: the contiguous device run differs from the host interpreter"

    return check


@pytest.mark.parametrize("kind", VC.ALL_KINDS)
def test_sampler_sample_euler_with_a_noise_tensor(kind):
    "three operands to vary: each of sample, prediction, noise alone as the view, then all three (fp32: the fused form; bf16 / fp16: the op tape)"
    smp, model, sched = PT.Euler(stochasticity=1), PM.NoiseModel(), PS.Scaled()
    for shape in VC.SHAPES:
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            subsets = [None] if kind in VC.PAIR_KINDS or kind in VC.MIXED else [("sample",), ("prediction",), ("noise",), None]
            for roles in subsets:
                before = native.launches
                oracle = None
                if roles is None:
                    oracle = euler_oracle if dtype == torch.float32 else tape_oracle(smp, model, sched, True)
                VC.sampler_pair(smp, model, sched, shape, dtype, DEV, kind, 1, steps=2, noise=True, roles=roles, oracle=oracle)
                # the route the contiguous run takes is the route the view run takes: both on the tape (16-bit) or neither (fp32)
                assert native.launches - before == (0 if dtype == torch.float32 else 4), (kind, dtype, roles, native.launches - before)


@pytest.mark.parametrize("kind", VC.ALL_KINDS)
@pytest.mark.parametrize("name", ["dpm2", "adams3", "unipc2"])
def test_sampler_sample_multistep_with_records_made_from_views(name, kind):
    smp = {"dpm2": PT.DPM(order=2), "adams3": PT.Adams(order=3), "unipc2": PT.UniPC(order=2)}[name]
    for shape in VC.SHAPES:
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            oracle = tape_oracle(smp, PM.NoiseModel(), PS.Scaled(), False) if dtype != torch.float32 and kind == "sliced" else None
            VC.sampler_pair(smp, PM.NoiseModel(), PS.Scaled(), shape, dtype, DEV, kind, 2, steps=4, oracle=oracle)


def test_sampler_sample_float64():
    for kind in ("sliced", "offset_small", "channels_last_offset"):
        VC.sampler_pair(PT.DPM(order=2), PM.VelocityModel(), PS.ZSNR(), (2, 4, 5, 7), torch.float64, DEV, kind, 3, steps=3)


def test_chunk_second_of_a_280_byte_sample():
    "the `uncond, cond = noise_pred.chunk(2)` idiom at (1, 4, 5, 7): a bf16 half is 280 bytes, the second half sits 8 bytes past a 16-byte line"
    v = VC.chunk_second(VC.values(VC.CHUNK_SHAPE, torch.bfloat16, DEV, 0))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    for dtype in (torch.bfloat16, torch.float32):
        VC.sampler_pair(PT.DPM(order=2), PM.NoiseModel(), PS.Scaled(), VC.CHUNK_SHAPE, dtype, DEV, "chunk_second", 4, steps=3)


# ---- entry 2: whole wrapper runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["a", "c"])
@pytest.mark.parametrize("kind", VC.ALL_KINDS)
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_runs(name, kind, schedule):
    mk = WRAPPERS[name][0]
    for shape in VC.SHAPES:
        for dtype, scale in CONFIGS:
            oracle = step_oracle(name, dtype) if name != "dpm3_sde" and scale is not None and kind == "sliced" and schedule == "a" else None
            VC.run_pair(lambda: mk(compute_scale=scale), shape, dtype, DEV, VC.plan_of(schedule, kind, STEPS), 5, oracle=oracle, label=f"{name}/{scale}/{schedule}")
        # invert_prediction without a compute scale: the negated prediction is a tape expression of its own in front of the step
        VC.run_pair(lambda: mk(compute_scale=None, invert_prediction=True), shape, torch.bfloat16, DEV, VC.plan_of(schedule, kind, STEPS), 5, label=f"{name}/inverted/{schedule}")


@pytest.mark.parametrize("steps", [STEPS, 10])
@pytest.mark.parametrize("kind", VC.ALL_KINDS)
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_run_that_meets_views_after_its_steps_were_learned(name, kind, steps):
    """schedule (b): run 1 on contiguous tensors learns the step programs and the replayed entries; after set_timesteps, run 2 hands views
    to steps 2 and 4.  The replay counters show the guard was in play: the contiguous run replays every step it can, the view run exactly
    the steps whose history window holds no record made from a view (a replayed step binds its history by pointer).  The 10-step run
    leaves room behind the views for the history of every sampler here to run clean again."""
    mk = WRAPPERS[name][0]
    keep = mk().sampler.require_previous
    plan = VC.plan_of("b", kind, steps)
    for shape in VC.SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            notes = VC.run_pair(mk, shape, dtype, DEV, plan, 7, warm_run=True, label=f"{name}/b{steps}")
            view, full = VC.expected_replays(keep, notes["bindable"])
            note_margin("operand views replay", f"{name} {steps} steps {kind} {shape}: replayed steps of the view run", notes["hits_view"], None)
            note_margin("operand views replay", f"{name} {steps} steps {kind} {shape}: replayed steps of the contiguous run", notes["hits_contiguous"], None)
            assert notes["hits_view"] <= notes["hits_contiguous"]
            if mk().sampler.require_noise and (shape[1] * shape[2] * shape[3]) % 8:
                continue  # (a draw that cannot be fused is a noise TENSOR among the operands: such steps are not replayed at all; counters recorded only)
            assert notes["hits_contiguous"] == full > 0, (name, kind, shape, dtype, notes["hits_contiguous"], full)
            assert notes["hits_view"] == view, (name, kind, shape, dtype, notes["hits_view"], view)


@pytest.mark.parametrize("kind", ["offset_8", "sliced", "channels_last_offset", "sample_offset_8+output_sliced"])
@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_that_met_views_in_its_first_run(name, kind):
    """the other order: the wrapper's FIRST run is on views, so whatever a step launched over temporaries (aligned copies, contiguous copies)
    left behind -- a step program, a replayed entry -- must not be bound in run 2, which alternates views and contiguous tensors"""
    mk = WRAPPERS[name][0]
    for shape in VC.SHAPES[:2]:
        for dtype in (torch.float32, torch.bfloat16):
            VC.run_pair(mk, shape, dtype, DEV, VC.plan_of("c", kind, STEPS), 16, warm_run="views", label=f"{name}/views first")


@pytest.mark.parametrize("kind", ["sliced", "offset_8", "channels_last"])
@pytest.mark.parametrize("name", ["dpm3_sde", "adams4", "unipc3"])
def test_wrapper_run_on_views_of_buffers_refilled_in_place(name, kind):
    for shape in VC.SHAPES[:2]:
        for dtype in (torch.float32, torch.bfloat16):
            VC.reused_buffer_pair(WRAPPERS[name][0], shape, dtype, DEV, kind, 15)


# ---- entry 3: step_guided ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("kind", GUIDED_KINDS)
@pytest.mark.parametrize("name", ["euler", "dpm3_sde", "unipc3"])
def test_step_guided(name, kind, rescale):
    "guided calls on views, mixed with plain step() calls in one run (steps 1 and 4 are plain, on sliced operands)"
    mk = WRAPPERS[name][0]
    for shape in (VC.CHUNK_SHAPE, *VC.SHAPES):
        for dtype in (torch.bfloat16, torch.float32):
            plan = [GUIDED_KINDS[kind] if i not in (1, 4) else "sliced" for i in range(STEPS)]
            VC.run_pair(mk, shape, dtype, DEV, plan, 6, guided=lambda i: None if i in (1, 4) else 5.5, rescale=rescale, label=f"guided {name}/{kind}")


@pytest.mark.parametrize("rescale", [0.0, 0.7])
@pytest.mark.parametrize("kind", GUIDED_KINDS)
def test_step_guided_fp16(kind, rescale):
    """in fp16 the fused guided step and the guidance-only route need not agree bit for bit, and a view may send a call from
    one to the other.  One guided Euler step per case under the suite's no_further_from_exact rule: the view run is no further from the
    float64 evaluation of the three guidance lines (and rescale_noise_cfg's four) plus the step than the contiguous run; both distances
    are recorded."""
    scale = 5.5

    def exact_for(steps):
        driver = OW.StepDriver(OA.make("euler"), OS.scaled(), "eps", compute=torch.float64)
        driver.set_timesteps(steps)

        def exact(i, t, ops):
            u, c, x = (ops[r].cpu().double() for r in ("uncond", "cond", "sample"))
            p = u + scale * (c - u)
            if rescale:
                dims = list(range(1, p.ndim))
                p = rescale * (p * (c.std(dim=dims, keepdim=True) / p.std(dim=dims, keepdim=True))) + (1 - rescale) * p
            return driver.step(p, t, x)  # (prev_sample, pred_original_sample: the guided prediction itself)

        return exact

    for shape in (VC.CHUNK_SHAPE, *VC.SHAPES[:2]):
        VC.run_pair(WRAPPERS["euler"][0], shape, torch.float16, DEV, [GUIDED_KINDS[kind]], 8, guided=lambda i: scale, rescale=rescale, exact=exact_for(STEPS),
                            run_steps=STEPS, label=f"fp16 guided {kind} rescale {rescale} {shape}")


# ---- entry 4: in-painting ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("expanded", "offset_8", "sliced"), ("expanded", "sliced", "offset_8"), ("expanded", "channels_last", "channels_last")], ids="+".join)
@pytest.mark.parametrize("name", ["euler", "dpm3_sde", "unipc3"])
def test_inpaint(name, kinds):
    """set_inpaint(mask, original_samples, noise) with an `expand`ed one-channel mask; the steps behind it run on view latents.  With
    original_samples, noise, latents and model outputs all channels-last a deterministic single-output sampler is the documented
    one-launch case: prev_sample is channels-last (clause 4, asserted by run_pair)."""
    mk = WRAPPERS[name][0]
    latents = "channels_last" if kinds[1] == "channels_last" else "sliced"
    for shape in VC.SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            for schedule in ("a", "c"):
                VC.run_pair(mk, shape, dtype, DEV, VC.plan_of(schedule, latents, STEPS), 9, inpaint=kinds, label=f"inpaint {name}/{'+'.join(kinds)}/{schedule}")


# ---- entry 5: Runge-Kutta stages ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", VC.ALL_KINDS)
def test_rk_wrapper_views_at_stage_two(kind):
    check_rk(DEV, kind, VC.SHAPES)


# ---- entry 6: noise and model transforms on 16-bit tensors (tape entries) -----------------------------------------------------------------
@pytest.mark.parametrize("kind", VC.ALL_KINDS)
def test_noise_and_model_transforms(kind):
    check_transforms(DEV, kind, (torch.bfloat16, torch.float16, torch.float32))


# ---- entry 7: generators on a caller's tensor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sliced", "offset_small"])
def test_colorize_noise_on_a_view(kind):
    from test_noise_gpu import TOL

    for shape in ((4, 16, 16), (3, 10, 12)):
        for dtype in (torch.float32, torch.bfloat16):
            white = VC.values(shape, dtype, DEV, 12)
            view = VC.KINDS[kind](white)
            watch = VC.Watch(view)
            got = PN.Colored.colorize_noise(view, exponent=1.0, energy=1.5)
            ref = PN.Colored.colorize_noise(VC.twin(view), exponent=1.0, energy=1.5)
            what = f"colorize_noise {shape} {dtype} {kind}"
            assert VC.same_bits(got, ref), what
            watch.assert_untouched(what)
            watch.assert_engine_owned(got, what)
            if dtype == torch.float32:  # the contiguous call against the oracle, at the generators' bar
                want = ON.colorize(white.cpu(), exponent=1.0, energy=1.5)
                err = ((ref.cpu().double() - want.double()).abs().max() / want.double().abs().max()).item()
                assert note_margin("operand views colorize", "contiguous call vs oracle", err, TOL) <= TOL, (what, err)


@pytest.mark.parametrize("kind", ["permuted_other", "sliced", "offset_small", "channels_last"])
def test_power_blend_on_views(kind):
    for shape in VC.SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            vals = {"a": VC.values(shape, dtype, DEV, 13), "b": VC.values(shape, dtype, DEV, 14)}
            ops = VC.build(kind, vals)
            watch = VC.Watch(*ops.values())
            got = lazy.power_blend(ops["a"], ops["b"], 0.6, 0.4, 0.5)
            ref = lazy.power_blend(VC.twin(ops["a"]), VC.twin(ops["b"]), 0.6, 0.4, 0.5)
            what = f"power_blend {shape} {dtype} {kind}"
            assert VC.same_bits(got, ref), what
            watch.assert_untouched(what)
            watch.assert_engine_owned(got, what)
            assert got.is_contiguous(), what


# ---- entry 8: autograd --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inpaint", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("kind", ["sliced", "offset_small"])
def test_autograd_through_a_wrapper_step(kind, inpaint):
    for dtype in (torch.float32, torch.bfloat16):
        grads = check_autograd(DEV, kind, dtype, inpaint=inpaint)
        if not inpaint:  # the contiguous device run against torch.autograd of the host run (a masked host step has no backward)
            host = check_autograd(torch.device("cpu"), kind, dtype)
            for k, (g, h) in enumerate(zip(grads, host)):
                assert_close(g, h, dtype, f"autograd {kind} {dtype} leaf {k}: device grad vs host autograd")


# ---- entry 9: the entries that refuse (clause 2) ------------------------------------------------------------------------------------------
def rolling_state(batch):
    return (batch.ticks, tuple(batch.index_vector()), len(batch._outputs), tuple(None if r is None else r.position for r in batch._requests))


@pytest.mark.parametrize("case", VC.REFUSES)
def test_rolling_batch_refuses_a_sliced_operand_and_nothing_changes(case):
    from skrample_amd.rolling import RollingBatch

    exc, names = VC.REFUSES[case]
    guided = "step_guided" in case
    unit, capacity = (8, 16, 16), 2
    mk = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled())  # noqa: E731
    example = torch.zeros((capacity, *unit), dtype=torch.bfloat16, device=DEV)
    seen, clean = (RollingBatch(mk, example, capacity=capacity, guided=guided) for _ in range(2))
    x = VC.values(unit, torch.bfloat16, DEV, 20)
    for b in (seen, clean):
        b.admit(0, x.clone(), mk(), 4, **({"guidance_scale": 3.0} if guided else {}))
    u, c = VC.values((capacity, *unit), torch.bfloat16, DEV, 21), VC.values((capacity, *unit), torch.bfloat16, DEV, 22)
    bad = VC.sliced(u if "uncond" in case or not guided else c)
    watch, before = VC.Watch(bad), rolling_state(seen)
    with pytest.raises(exc, match=names):
        if not guided:
            seen.step(bad)
        elif "uncond" in case:
            seen.step_guided(bad, c)
        else:
            seen.step_guided(u, bad)
    assert rolling_state(seen) == before, "a refused tick changed the batch's state"
    watch.assert_untouched(case)
    for tick in range(2):  # the next valid calls have the bits of a batch that never saw the bad one
        for b in (seen, clean):
            b.step_guided(u.clone(), c.clone()) if guided else b.step(u.clone())
        torch.cuda.synchronize()
        assert VC.same_bits(seen.latents, clean.latents), (case, tick)
    assert rolling_state(seen) == rolling_state(clean)


def test_capture_sampling_loop_normalises_a_non_contiguous_example():
    """capture_sampling_loop documents no refusal -- `example` fixes shape, dtype and device -- and clones the example into its static
    buffer: a sliced example and sliced latents give the loop of the contiguous example, bit for bit, and stay untouched"""
    from skrample_amd.graphs import capture_sampling_loop

    shape, steps = (2, 4, 16, 16), 3
    net = lambda x, t: x * 0.75 - (t / 2000) * x.abs()  # noqa: E731
    mk = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled())  # noqa: E731
    x0 = VC.values(shape, torch.float32, DEV, 23)
    view = VC.sliced(x0)
    watch = VC.Watch(view)
    loop_v = capture_sampling_loop(mk(), net, view, steps)
    loop_c = capture_sampling_loop(mk(), net, VC.twin(view), steps)
    got, ref = loop_v(view).clone(), loop_c(VC.twin(view)).clone()
    torch.cuda.synchronize()
    assert VC.same_bits(got, ref)
    watch.assert_untouched("capture_sampling_loop")
    watch.assert_engine_owned(got, "capture_sampling_loop")
