"""Parity of the HIP path against the oracle and the reference-derived fixtures (needs an MI355X).

Bars (BASELINE.md / north_star): fp32 outputs  ||hip - ref||_inf / ||ref||_inf <= 1e-5 ;
bf16 / fp16 outputs within 1 unit in the last place of the reference's (fp32-computed, once-rounded)
result.  All launches go through the C-ABI (skr_step_launch) -- there is no other execution path.
"""

import ctypes
import itertools

import zlib

import numpy as np
import pytest
import torch
from cases import MODELS, NATIVE16_ORACLE, NATIVE16_TAGS, SAMPLERS, SCHEDULES, bf16_ulp, from_bits, native16_case, oracle_schedule
from conftest import note_margin, load_npz

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skr_oracle import noise as ON
from skr_oracle import rk as OK
from skr_oracle import samplers as OA
from skr_oracle import schedules as OS
from skr_oracle import wrapper as OW
from skrample_amd import _hip
from skrample_amd.pytorch import noise as PN
from skrample_amd.sampling import lazy
from skrample_amd.sampling import models as PM
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
REL_TOL_F32 = 1e-5  # stated tolerance for floating-point parity (north_star)
# 16-bit results: "within 1 unit in the last place of the reference's result" needs an additive term for elements that are cancellation
# residues (their last place is far below the fp32 rounding noise of their terms).  Round 3 allowed 1e-5 * max|ref| for it without a
# measured number; measured over every 16-bit comparison of the GPU and CPU suites (profiles/r04_parity_margins.txt): at most 8.6e-8 *
# max|ref| on bf16 results (640 comparisons), 2.8e-8 on fp16 (220), 0 through the host executor.  The term is 1e-6 now.
ADDITIVE_16 = 1e-6


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


class Injected:
    "stands in for BatchTensorNoise: replays given noise tensors (what the reference consumed)"

    def __init__(self, draws, device):
        self.draws = [d.to(device) for d in draws]

    def generate(self, step):
        return self.draws.pop(0)

    generate_lazy = generate


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def assert_close(got, ref, dtype, what="", flips=0.05):
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, got.shape)
    g, r = got.detach().cpu(), ref.detach().cpu()
    assert torch.isfinite(g.float()).all(), what
    family = "step " + str(dtype).replace("torch.", "")
    if dtype in (torch.float32, torch.float64):
        assert note_margin(family, "rel inf-norm error", rel_err(g, r), REL_TOL_F32) <= REL_TOL_F32, (what, rel_err(g, r))
    else:
        # 1 unit in the last place of the reference, plus the fp32 tolerance on the scale of the operands
        # (results near zero come from cancellation: their ulp is far below the fp32 noise floor of the terms)
        ulp = bf16_ulp(r) * (1 if dtype == torch.bfloat16 else 2.0**-3)  # fp16 has 3 more mantissa bits
        diff = (g.float() - r.float()).abs()
        scale = r.float().abs().max().clamp_min(1e-30)
        # what is MEASURED: the worst difference in last-place units, how much of the additive term an element needed beyond its one
        # unit (as a fraction of max|ref|; the bar allows REL_TOL_F32), and the share of elements that differ at all
        big = r.float().abs() >= 1e-3 * scale  # (an element that is a cancellation residue has a last place far below the fp32 noise of its terms)
        note_margin(family, "max |diff| in units of the reference's last place (elements >= 1e-3 max|ref|)", (diff[big] / ulp[big]).max().item() if big.any() else 0.0, None)
        note_margin(family, "max (|diff| - 1 ulp) / max|ref|", ((diff - ulp).clamp_min(0).max() / scale).item(), ADDITIVE_16)
        note_margin(family, "share of elements differing in the last place", (g != r).float().mean().item(), flips)
        bad = diff > ulp + ADDITIVE_16 * scale
        assert not bad.any(), (what, int(bad.sum()), diff.max().item())
        assert (g != r).float().mean().item() < flips, (what, "too many last-place flips", (g != r).float().mean().item())


# ---- reference fixtures through the scheduler wrapper ---------------------------------------------------
FIXTURE_WRAPPERS = {
    "cfg1": (lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled()), torch.float32),
    "cfg2": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled())), torch.bfloat16),
    "cfg3": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Linear(), PM.FlowModel()), torch.bfloat16),
    "cfg4": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.ZSNR(), PM.VelocityModel()), torch.bfloat16),
    "cfg5": (lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=6, stochasticity=1), torch.bfloat16),
}
EXTRA_WRAPPERS = {
    "euler_sde_v_zsnr": (lambda: PD.SkrampleWrapperScheduler(PT.Euler(stochasticity=1), PS.ZSNR(), PM.VelocityModel()), torch.bfloat16),
    "dpm1_ode_eps": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=1), PS.Scaled()), torch.bfloat16),
    "dpm3_sde_eps": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=3, stochasticity=0.5), PS.Scaled()), torch.float32),
    "dpm2_flow_shift": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.FlowShift(PS.Linear()), PM.FlowModel()), torch.bfloat16),
    "adams9_data": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=9), PS.Scaled(), PM.DataModel()), torch.float32),
    "unip4_eps": (lambda: PD.SkrampleWrapperScheduler(PT.UniP(order=4, stochasticity=-1.5), PS.Scaled()), torch.float32),
    "unipc2_fast_v": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=2, fast_solve=True), PS.Scaled(), PM.VelocityModel()), torch.bfloat16),
    "unipc3_adams_pred": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, predictor=PT.Adams(order=2)), PS.Linear(), PM.FlowModel()), torch.float32),
    "dpm2_deriv_v": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, derivative_transform=PM.VelocityModel()), PS.Scaled()), torch.float32),
    "adams3_noderiv": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=3, derivative_transform=None), PS.Scaled()), torch.float32),
    "euler_invert": (lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled(), invert_prediction=True), torch.bfloat16),
    "dpm2_f16": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Scaled()), torch.float16),
    "dpm2_f64": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Scaled(), compute_scale=torch.float64), torch.float64),
    "rku2_ode_flow": (lambda: PD.RKUltraWrapperScheduler(PS.Linear(), sampler_order=2, model=PM.FlowModel()), torch.bfloat16),
    "rku4_sde_v": (lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=4, stochasticity=0.5, model=PM.VelocityModel()), torch.float32),
    "rku5_noderiv": (lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=5, derivative_transform=None), torch.float32),
}

# round 2 (tests/golden/steps_extra2.npz): the predictor-corrector blend, DynasauRK, nested predictors, the other sub-schedules
EXTRA2_WRAPPERS = {
    "spc_default": (lambda: PD.SkrampleWrapperScheduler(PT.SPC(), PS.Scaled()), torch.bfloat16),
    "spc_power2_bias": (lambda: PD.SkrampleWrapperScheduler(PT.SPC(power=2, bias=0.3, adaptive=False), PS.Scaled()), torch.float32),
    "spc_invert_dpm_unip": (lambda: PD.SkrampleWrapperScheduler(PT.SPC(predictor=PT.DPM(order=2), corrector=PT.UniP(order=3), invert=True), PS.Karras(PS.Scaled())), torch.float32),
    "spc_sde_v": (lambda: PD.SkrampleWrapperScheduler(PT.SPC(predictor=PT.Euler(stochasticity=1)), PS.ZSNR(), PM.VelocityModel()), torch.bfloat16),
    "spc_flow_power_half": (lambda: PD.SkrampleWrapperScheduler(PT.SPC(power=0.5, bias=-0.2), PS.Linear(), PM.FlowModel()), torch.float32),
    "unipc3_dpm_pred_sde": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1, predictor=PT.DPM(order=2, stochasticity=1)), PS.Karras(PS.Scaled())), torch.bfloat16),
    "dpm2_exponential": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Exponential(PS.Scaled())), torch.float32),
    "adams2_beta_zsnr": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=2), PS.Beta(PS.ZSNR()), PM.VelocityModel()), torch.float32),
    "euler_probit_flow": (lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Probit(PS.Linear()), PM.FlowModel()), torch.bfloat16),
    "dpm2_hyper": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=0.3), PS.Hyper(PS.Scaled())), torch.float32),
    "unip2_sinner_flow": (lambda: PD.SkrampleWrapperScheduler(PT.UniP(order=2), PS.Sinner(PS.Linear()), PM.FlowModel()), torch.float32),
    "dyn3_flow": (lambda: PD.DynasauRKWrapperScheduler(PS.Linear(), sampler_order=3, model=PM.FlowModel()), torch.float32),
    "dyn2_sde_eps": (lambda: PD.DynasauRKWrapperScheduler(PS.Scaled(), sampler_order=2, stochasticity=0.5), torch.bfloat16),
    "dyn4_v": (lambda: PD.DynasauRKWrapperScheduler(PS.Scaled(), sampler_order=4, model=PM.VelocityModel()), torch.float32),
}


# round 3 (tests/golden/steps_extra3.npz): the high orders, on one 2048-element sample -> the compile-time kernels of 10-22 operands
EXTRA3_WRAPPERS = {
    "unipc6_sde_eps": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=6, stochasticity=1), PS.Scaled()), torch.bfloat16),
    "adams9_eps_karras": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=9), PS.Karras(PS.Scaled())), torch.bfloat16),
    "adams6_v_zsnr": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=6), PS.ZSNR(), PM.VelocityModel()), torch.bfloat16),
    "unip7_flow": (lambda: PD.SkrampleWrapperScheduler(PT.UniP(order=7), PS.Linear(), PM.FlowModel()), torch.float32),
    "unipc9_flow": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=9), PS.Linear(), PM.FlowModel()), torch.bfloat16),
}


# round 5 (tests/golden/steps_extra4.npz): compute_scale=float64 over 16-bit latents (fp64 accumulation, one rounding to the 16-bit result)
EXTRA4_WRAPPERS = {
    "dpm2_f64_bf16": (lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Scaled(), compute_scale=torch.float64), torch.bfloat16),
    "unipc3_f64_f16": (lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Linear(), PM.FlowModel(), compute_scale=torch.float64), torch.float16),
    "adams4_f64_bf16": (lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.ZSNR(), PM.VelocityModel(), compute_scale=torch.float64), torch.bfloat16),
    "rku4_f64_bf16": (lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=4, stochasticity=0.5, compute_scale=torch.float64), torch.bfloat16),
}


def replay_fixture(w, fx, dtype, dev, name, exact=False, steps=None):
    "teacher-forced replay: every step sees exactly the inputs the reference saw (exact: results must equal the reference's bit for bit)"
    n_calls = len(fx["timesteps"])
    w.set_timesteps(steps if steps is not None else n_calls if not isinstance(w, PD.RKWrapperCore) else 3)
    np.testing.assert_allclose(w.timesteps.numpy(), fx["timesteps"], rtol=0, atol=1e-9)
    used = int(fx["noise_used"])
    w._noise_generator = Injected([torch.from_numpy(v) for v in fx["noises"][:used]], dev) if used else None
    x = from_bits(fx["x0"], dtype).to(dev)
    for i, t in enumerate(w.timesteps):
        out = from_bits(fx["outs"][i], dtype).to(dev)
        prev, pred = w.step(out, t, x, return_dict=False)
        pred = torch.as_tensor(pred.materialize() if isinstance(pred, lazy.LazyTensor) else pred)
        assert_close(prev, from_bits(fx["prev"][i], dtype), dtype, f"{name} step {i} prev_sample")
        assert_close(pred, from_bits(fx["pred"][i], dtype), dtype, f"{name} step {i} pred_original_sample")
        if exact:
            assert torch.equal(prev.cpu(), from_bits(fx["prev"][i], dtype)) and torch.equal(pred.cpu(), from_bits(fx["pred"][i], dtype)), (name, i)
        x = from_bits(fx["prev"][i], dtype).to(dev)
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


@pytest.mark.parametrize("name", FIXTURE_WRAPPERS)
def test_baseline_config_fixtures(name, dev):
    "the five BASELINE.json configs (reduced shape): HIP wrapper vs outputs of the reference itself"
    mk, dt = FIXTURE_WRAPPERS[name]
    replay_fixture(mk(), load_npz(f"steps_{name}.npz"), dt, dev, name)


@pytest.mark.parametrize("name", EXTRA_WRAPPERS)
def test_extra_fixtures(name, dev):
    blob = load_npz("steps_extra.npz")
    fx = {k.split("/", 1)[1]: v for k, v in blob.items() if k.startswith(name + "/")}
    mk, dt = EXTRA_WRAPPERS[name]
    replay_fixture(mk(), fx, dt, dev, name)


@pytest.mark.parametrize("name", EXTRA2_WRAPPERS)
def test_extra2_fixtures(name, dev):
    blob = load_npz("steps_extra2.npz")
    fx = {k.split("/", 1)[1]: v for k, v in blob.items() if k.startswith(name + "/")}
    mk, dt = EXTRA2_WRAPPERS[name]
    replay_fixture(mk(), fx, dt, dev, name)


@pytest.mark.parametrize("name", EXTRA4_WRAPPERS)
def test_float64_compute_scale_on_16_bit_latents(name, dev):
    """compute_scale=torch.float64 with bf16 / fp16 tensors (reference diffusers.py:575-599): 16-bit operands widened exactly, accumulated in
    double, rounded once (through fp32, as torch's double -> bf16 / half conversion does) -- the reference's recorded results come back bit for bit."""
    blob = load_npz("steps_extra4.npz")
    fx = {k.split("/", 1)[1]: v for k, v in blob.items() if k.startswith(name + "/")}
    mk, dt = EXTRA4_WRAPPERS[name]
    replay_fixture(mk(), fx, dt, dev, name, exact=True)


# round 5 (tests/golden/steps_sweep.npz): 64 seeded random configurations stepped through the imported reference, each stored with the
# text of its constructor (W = diffusers module, T = samplers, S = schedules, M = models)
SWEEP_NAMES = {"W": PD, "T": PT, "S": PS, "M": PM, "torch": torch}
SWEEP_COUNT = 64


def sweep_case(index):
    import json

    blob = load_npz("steps_sweep.npz")
    meta = json.loads(str(blob["meta"]))
    assert len(meta) == SWEEP_COUNT
    m = meta[index]
    fx = {k.split("/", 1)[1]: v for k, v in blob.items() if k.startswith(m["tag"] + "/")}
    return m, fx, getattr(torch, m["dtype"])


@pytest.mark.parametrize("index", range(SWEEP_COUNT))
def test_reference_recorded_random_sweep(index, dev):
    """sampler x nesting x schedule x modifier x predictor x eta x dtype x compute_scale x ragged shape x run length, drawn from a seeded
    generator and stepped through the reference itself (tools/make_golden.py::sweep): the wrapper on the device, teacher-forced"""
    m, fx, dt = sweep_case(index)
    replay_fixture(eval(m["text"], SWEEP_NAMES), fx, dt, dev, m["text"], steps=m["steps"])


NATIVE_SWEEP_COUNT = 32


def replay_native_sweep(index, dev):
    """tests/golden/steps_sweep_native.npz: the sweep grammar under compute_scale=None on 16-bit tensors, where the reference computes in the tensor
    dtype one rounded op at a time (Runge-Kutta wrappers, invert_prediction, nested predictors, derivative transforms) -- bit for bit"""
    import json

    blob = load_npz("steps_sweep_native.npz")
    meta = json.loads(str(blob["meta"]))
    assert len(meta) == NATIVE_SWEEP_COUNT
    m = meta[index]
    fx = {k.split("/", 1)[1]: v for k, v in blob.items() if k.startswith(m["tag"] + "/")}
    dt = getattr(torch, m["dtype"])
    w = eval(m["text"], SWEEP_NAMES)
    w.set_timesteps(m["steps"])
    np.testing.assert_allclose(w.timesteps.numpy(), fx["timesteps"], rtol=0, atol=1e-9)
    used = int(fx["noise_used"])
    w._noise_generator = Injected([from_bits(v, dt) for v in fx["noises"][:used]], dev) if used else None
    x = from_bits(fx["x0"], dt).to(dev)
    for i, t in enumerate(w.timesteps):
        prev, pred = w.step(from_bits(fx["outs"][i], dt).to(dev), t, x, return_dict=False)
        pred = torch.as_tensor(pred.materialize() if isinstance(pred, lazy.LazyTensor) else pred)
        for name, got, want in (("prev_sample", prev, fx["prev"][i]), ("pred_original_sample", pred, fx["pred"][i])):
            assert got.dtype == dt and torch.equal(got.cpu(), from_bits(want, dt)), (m["text"], i, name, (got.cpu().double() - from_bits(want, dt).double()).abs().max())
        x = prev


@pytest.mark.parametrize("index", range(NATIVE_SWEEP_COUNT))
def test_reference_recorded_sweep_without_a_compute_scale(index, dev):
    replay_native_sweep(index, dev)


def replay_native_api16(dev):
    """tests/golden/native_api16.npz: functional sampler loops (RKUltra, DynasauRK, the structured adapter), model transforms called directly and
    Point.add_noise / remove_noise on bf16 / fp16 tensors, recorded from the reference (generic tensor operators, every one rounded) -- bit for bit"""
    import json

    from skrample_amd.common import DeltaPoint, Point
    from skrample_amd.sampling import functional as PF
    from skrample_amd.sampling import interface as PI

    blob = load_npz("native_api16.npz")
    names = {"F": PF, "I": PI, "T": PT, "S": PS, "M": PM, "Point": Point, "DeltaPoint": DeltaPoint}
    # the recording's network is `xx * factor` on CPU tensors: fp32 product, rounded to fp32, then to the tensor dtype.  torch's DEVICE kernel for an fp16
    # tensor times a Python number rounds once (the compiler folds the product and the conversion into v_fma_mixlo_f16), so a product that lands on a tie
    # in fp32 comes out one ulp away from the CPU's: spelled in fp32 steps the network is the same function on either side
    net = lambda xx, t, sg, al: (xx.float() * (0.3 - 0.1 * sg + 0.05 * al)).to(xx.dtype)  # noqa: E731
    checked = 0
    for m in json.loads(str(blob["meta"])):
        dt = torch.bfloat16 if m["dtype"] == "bf16" else torch.float16
        get = lambda key: torch.from_numpy(blob[f"{m['dtype']}/{key}"].copy()).view(dt)  # noqa: E731
        s_, o_, n_ = get("s").to(dev), get("o").to(dev), get("n").to(dev)
        want = torch.from_numpy(blob[m["key"]].copy()).view(dt)
        if m["kind"] == "loop":
            pool = [d.to(dev) for d in get("draws")]
            got = eval(m["sampler"], names).sample_model(s_.clone(), net, eval(m["model"], names), eval(m["schedule"], names), m["steps"], rng=lambda *_: pool.pop(0))
            assert len(get("draws")) - len(pool) == m["draws_used"], m
        else:
            got = eval(m["text"], {**names, "s": s_, "o": o_, "n": n_})
        got = torch.as_tensor(got.materialize() if isinstance(got, lazy.LazyTensor) else got).cpu()
        assert got.dtype == dt and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)), (m, (got.double() - want.double()).abs().max())
        checked += 1
    assert checked == 40


def test_reference_recorded_functional_loops_and_transforms_on_16_bit_tensors(dev):
    replay_native_api16(dev)


@pytest.mark.parametrize("name", EXTRA3_WRAPPERS)
def test_high_order_fixtures(name, dev):
    """Adams-Bashforth 6 / 9, UniP 7, UniPC 6 / 9 (north_star: "Adams-IPNDM 1-9"): outputs of the reference's own step() replayed
    through the wrapper; the launches are traced to make sure the late steps really take the compile-time one-trip kernels'
    operand counts (> 8 operands in one launch)."""
    blob = load_npz("steps_extra3.npz")
    fx = {k.split("/", 1)[1]: v for k, v in blob.items() if k.startswith(name + "/")}
    mk, dt = EXTRA3_WRAPPERS[name]
    w = mk()
    w.set_timesteps(len(fx["timesteps"]))
    _hip.trace = []
    try:
        # (tracing here only records; the wrapper's own program tracing is skipped while a trace list is installed)
        replay_fixture(w, fx, dt, dev, name)
        widest = max(plan.n_terms for plan, *_ in _hip.trace)
    finally:
        _hip.trace = None
    assert widest > 8, widest


# ---- every sampler x model on the GPU vs the oracle (fp32 in/out, injected noise) ---------------------------
@pytest.mark.parametrize("sampler", [s for s in SAMPLERS])
def test_samplers_vs_oracle(sampler, dev):
    mk_o, mk_p = SAMPLERS[sampler]
    steps, shape = 9, (3, 4, 24, 20)
    for sname, mname in (("karras_scaled", "eps"), ("linear", "flow"), ("zsnr", "v"), ("scaled", "data")):
        g = torch.Generator().manual_seed(zlib.crc32(f"{sampler}/{sname}".encode()))  # (str hashes change from process to process)
        w = PD.SkrampleWrapperScheduler(mk_p(), SCHEDULES[sname][1](), MODELS[mname][1])
        o = OW.StepDriver(mk_o(), oracle_schedule(sname, steps), MODELS[mname][0])
        w.set_timesteps(steps)
        o.set_timesteps(steps)
        noises = [torch.randn(shape, generator=g) for _ in range(steps)]
        w._noise_generator = Injected(noises, dev)
        x = torch.randn(shape, generator=g)
        for i, t in enumerate(w.timesteps):
            out = torch.randn(shape, generator=g)
            got = w.step(out.to(dev), t, x.to(dev), return_dict=False)[0]
            ref = o.step(out, t, x, noise=noises[i])[0]
            assert_close(got, ref, torch.float32, f"{sampler}/{sname}/{mname} step {i}")
            x = ref


FLOW_SCHEDULES = ("linear", "flowshift_linear", "sinner_linear", "probit_linear")
VP_SCHEDULES = ("scaled", "karras_scaled", "hyper_scaled", "exponential_scaled", "scaled_neg_b1", "zsnr", "beta_zsnr_flowshift")


@pytest.mark.parametrize("seed", range(48))
def test_random_sweep_vs_oracle(seed, dev):
    """seeded random draw over (sampler x schedule x predictor x tensor dtype x ragged shape x run length): the wrapper on
    the device against the oracle's StepDriver, teacher-forced, injected noise"""
    import random

    rng = random.Random(1000 + seed)
    sampler = rng.choice(sorted(SAMPLERS))
    mk_o, mk_p = SAMPLERS[sampler]
    if rng.random() < 0.4:
        sname, mname = rng.choice(FLOW_SCHEDULES), rng.choice(("flow", "data", "v"))
    else:
        sname = rng.choice(VP_SCHEDULES)
        mname = rng.choice(("v", "data") if sname in ("zsnr", "beta_zsnr_flowshift") else ("eps", "v", "data"))
    dtype = rng.choice((torch.float32, torch.float32, torch.bfloat16, torch.float16))
    shape = (rng.randint(1, 3), rng.randint(1, 5), rng.choice((8, 13, 16, 31)), rng.choice((8, 10, 24, 17)))
    steps = rng.randint(2, 12)
    g = torch.Generator().manual_seed(seed)
    w = PD.SkrampleWrapperScheduler(mk_p(), SCHEDULES[sname][1](), MODELS[mname][1])
    o = OW.StepDriver(mk_o(), oracle_schedule(sname, steps), MODELS[mname][0])
    w.set_timesteps(steps)
    o.set_timesteps(steps)
    np.testing.assert_allclose(w.timesteps.numpy(), o.timesteps.numpy(), rtol=0, atol=1e-9)
    noises = [torch.randn(shape, generator=g) for _ in range(steps)]
    w._noise_generator = Injected(noises, dev)
    x = torch.randn(shape, generator=g).to(dtype)
    what = f"{sampler}/{sname}/{mname}/{dtype}/{shape}/{steps}"
    for i, t in enumerate(w.timesteps):
        out = torch.randn(shape, generator=g).to(dtype)
        try:
            ref = o.step(out, t, x, noise=noises[i])[0]
        except ZeroDivisionError:  # degenerate schedule (e.g. all points equal): the reference's arithmetic raises, so must ours
            with pytest.raises(ZeroDivisionError):
                w.step(out.to(dev), t, x.to(dev), return_dict=False)
            return
        got = w.step(out.to(dev), t, x.to(dev), return_dict=False)[0]
        if not torch.isfinite(ref.float()).all():  # a degenerate pairing (e.g. division by alpha = 0): nothing to compare
            return
        assert_close(got, ref, dtype, f"{what} step {i}")
        x = ref


def chunked_sweep_case(seed: int, dev) -> None:
    """one seeded draw over (sampler x schedule x predictor x dtype x run length) on shapes made of whole 2048-element chunks --
    the domain of the one-trip kernels (k1 / k2) -- with the step noise drawn INSIDE the kernel: checked step by step against the
    oracle fed the Philox normals the specification assigns (stream 256 * draw)"""
    import random

    rng = random.Random(7000 + seed)
    sampler = rng.choice(sorted(SAMPLERS))
    mk_o, mk_p = SAMPLERS[sampler]
    if rng.random() < 0.4:
        sname, mname = rng.choice(FLOW_SCHEDULES), rng.choice(("flow", "data", "v"))
    else:
        sname = rng.choice(VP_SCHEDULES)
        mname = rng.choice(("v", "data") if sname in ("zsnr", "beta_zsnr_flowshift") else ("eps", "v", "data"))
    dtype = rng.choice((torch.float32, torch.bfloat16, torch.bfloat16, torch.float16))
    batch = rng.randint(1, 3)
    chunks = rng.choice((1, 2, 3, 4, 6, 9))  # chunks per sample: powers of two (shift) and others (division)
    shape = (batch, chunks * 2, 32, 32)
    steps = rng.randint(2, 10)
    seeds = [rng.randrange(2**62) for _ in range(batch)]
    g = torch.Generator().manual_seed(seed)
    w = PD.SkrampleWrapperScheduler(mk_p(), SCHEDULES[sname][1](), MODELS[mname][1])
    o = OW.StepDriver(mk_o(), oracle_schedule(sname, steps), MODELS[mname][0])
    w.set_timesteps(steps)
    o.set_timesteps(steps)
    x = torch.randn(shape, generator=g).to(dtype)
    n = shape[1] * shape[2] * shape[3]
    what = f"{sampler}/{sname}/{mname}/{dtype}/{shape}/{steps}"
    draws = 0
    for i, t in enumerate(w.timesteps):
        out = torch.randn(shape, generator=g).to(dtype)
        noise = None
        if w.sampler.require_noise:
            noise = torch.from_numpy(np.stack([ON.philox_normal(sd, draws * 256, n) for sd in seeds])).reshape(shape)
            draws += 1
        try:
            ref = o.step(out, t, x, noise=noise)[0]
        except ZeroDivisionError:
            return
        if not torch.isfinite(ref.float()).all():
            return
        got = w.step(out.to(dev), t, x.to(dev), generator=seeds, return_dict=False)[0]
        assert_close(got, ref, dtype, f"{what} step {i}", flips=0.10)
        x = ref


@pytest.mark.parametrize("seed", range(24))
def test_chunked_shapes_sweep_vs_oracle(seed, dev):
    chunked_sweep_case(seed, dev)


def test_inner_boundary_sample_packed(dev):
    "StructuredSampler.sample on HIP tensors: aliases in the record, fresh result tensor, inputs untouched"
    sched, model = PS.Karras(PS.Scaled()), PM.NoiseModel()
    osched = OS.karras(OS.scaled())
    g = torch.Generator().manual_seed(3)
    x, out, xp, outp, nz = (torch.randn(2, 4, 16, 16, generator=g) for _ in range(5))
    xd, od = x.to(dev), out.to(dev)
    keep = (xd.clone(), od.clone())
    prev = PT.SKSamples(xp.to(dev), outp.to(dev), PT.Step.from_int(4, 20), None, None)
    rec = PT.DPM(order=2, stochasticity=1).sample(xd, od, PT.Step.from_int(5, 20), model, sched, nz.to(dev), [prev])
    assert rec.sample is xd and rec.prediction is od and rec.final.data_ptr() not in (xd.data_ptr(), od.data_ptr())
    assert torch.equal(xd, keep[0]) and torch.equal(od, keep[1])
    ref = OA.sample(OA.make("dpm", 2, eta=1), x, out, (5 / 20, 6 / 20), "eps", osched, nz, [OA.Rec(xp, outp, (4 / 20, 5 / 20))]).final
    assert_close(rec.final, ref, torch.float32, "DPM.sample")
    # model-level API
    p = sched.ipoint(0.3)
    assert_close(model.to_x(xd, od, p), (x - p.sigma * out) / p.alpha, torch.float32, "to_x")
    dp = PT.DeltaPoint(sched.ipoint(0.3), sched.ipoint(0.35))
    from skr_oracle import predictors as OP

    assert_close(model.forward(xd, od, dp, nz.to(dev), 1.0), OP.forward("eps", x, out, OS.karras(OS.scaled()).ipoint(0.3), OS.karras(OS.scaled()).ipoint(0.35), nz, 1.0), torch.float32, "forward")
    assert_close(sched.ipoint(0.3).add_noise(xd, od), x * p.alpha + out * p.sigma, torch.float32, "add_noise")


@pytest.fixture
def fused_mode():
    "sampler-level calls on 16-bit tensors through the fused kernel (native.mode = 'never'), as every call was before round 5"
    from skrample_amd.sampling import native

    before, native.mode = native.mode, "never"
    yield
    native.mode = before


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["dpm2_sde", "adams3", "euler"])
def test_sampler_level_api_on_16_bit_tensors(dtype, kind, dev, fused_mode):
    """Called directly (no wrapper), the reference's samplers compute in the TENSOR dtype, rounding after every op
    (structured.py:209-283 -- only its wrappers widen to compute_scale).  Since round 5 that call replays the reference's own
    sequence (sampling/native.py, tests below); with native.mode = "never" it takes the fused kernel, which accumulates the collapsed
    form in fp32 and rounds once.  Pinned here for that mode: the results differ by a few last-place units of the 16-bit type, and the
    fused result is never farther from the exact (fp64) answer than the reference's native-dtype chain is."""
    mk_o, mk_p = {"dpm2_sde": (OA.make("dpm", 2, eta=1), PT.DPM(order=2, stochasticity=1)), "adams3": (OA.make("adams", 3), PT.Adams(order=3)),
                  "euler": (OA.make("euler"), PT.Euler())}[kind]  # fmt: skip
    sched, model, osched = PS.Scaled(), PM.NoiseModel(), OS.scaled()
    g = torch.Generator().manual_seed(17)
    shape, steps = (2, 4, 16, 16), 12
    xs = [torch.randn(shape, generator=g).to(dtype) for _ in range(4)]
    outs = [torch.randn(shape, generator=g).to(dtype) for _ in range(4)]
    nzs = [torch.randn(shape, generator=g).to(dtype) for _ in range(4)]
    step_of = lambda i: (i / steps, (i + 1) / steps)  # noqa: E731
    hist = [(xs[k], outs[k], 5 + k) for k in range(3)]  # three earlier steps as history
    cur = 8
    prev_p = [PT.SKSamples(x.to(dev), o.to(dev), PT.Step.from_int(i, steps), None, None) for x, o, i in hist]
    got = mk_p.sample(xs[3].to(dev), outs[3].to(dev), PT.Step.from_int(cur, steps), model, sched, nzs[3].to(dev), prev_p).final.cpu()
    assert got.dtype == dtype
    native = OA.sample(mk_o, xs[3], outs[3], step_of(cur), "eps", osched, nzs[3], [OA.Rec(x, o, step_of(i)) for x, o, i in hist]).final
    exact = OA.sample(mk_o, xs[3].double(), outs[3].double(), step_of(cur), "eps", osched, nzs[3].double(), [OA.Rec(x.double(), o.double(), step_of(i)) for x, o, i in hist]).final
    assert native.dtype == dtype  # the oracle, like the reference, stayed in the tensor dtype
    ulp = bf16_ulp(exact.float()) * (1 if dtype == torch.bfloat16 else 2.0**-3)
    scale = exact.abs().max().item()
    err_engine = ((got.double() - exact).abs() / (ulp.double() + 1e-5 * scale)).max().item()
    err_native = ((native.double() - exact).abs() / (ulp.double() + 1e-5 * scale)).max().item()
    assert err_engine <= 0.51 + 1e-3, err_engine  # one rounding of the exact result (+ the fp32 noise floor of the operands)
    assert err_engine <= err_native + 1e-9  # never worse than the reference's own native-dtype chain ...
    assert ((got.double() - native.double()).abs() / (ulp.double() + 1e-5 * scale)).max().item() <= err_native + 0.51 + 1e-3  # ... and close to it


def native16_engine_vs_reference(tag, device):
    """The reference's recorded native-dtype chain (tests/golden/native16.npz) is 4-47 units away from the exact (fp64) result of
    the same inputs, a unit being the 16-bit ulp of the exact value + 1e-5 of its range; this engine, accumulating the collapsed
    form in fp32 and rounding once, stays within half a unit on every step -- never farther from exact than the reference is."""
    dt, steps, mname, sname, expr, t = native16_case(load_npz("native16.npz"), tag)
    sampler, sched, model = eval(expr, {"S": PT}), SCHEDULES[sname][1](), MODELS[mname][1]
    cfg, osched = NATIVE16_ORACLE[tag.split("/")[0]](OA), SCHEDULES[sname][0]()
    previous, exact_previous = [], []
    worst_engine = worst_reference = 0.0
    for i in range(steps):
        x, out, nz = t["x"][i], t["out"][i], t["noise"][i]
        rec = sampler.sample(x.to(device), out.to(device), PT.Step.from_int(i, steps), model, sched, nz.to(device) if sampler.require_noise else None, tuple(previous))
        assert rec.final.dtype == dt
        exact_rec = OA.sample(cfg, x.double(), out.double(), (i / steps, (i + 1) / steps), MODELS[mname][0], osched, nz.double() if OA.require_noise(cfg) else None, exact_previous)
        exact = exact_rec.final
        unit = (bf16_ulp(exact.float()) * (1 if dt == torch.bfloat16 else 2.0**-3)).double() + 1e-5 * exact.abs().max().item()
        worst_engine = max(worst_engine, ((torch.as_tensor(rec.final).double().cpu() - exact).abs() / unit).max().item())
        worst_reference = max(worst_reference, ((t["final"][i].double() - exact).abs() / unit).max().item())
        previous.append(rec)
        exact_previous.append(exact_rec)
        keep = sampler.require_previous
        previous = previous[max(len(previous) - keep, 0) :] if keep else []
        exact_previous = exact_previous[max(len(exact_previous) - keep, 0) :] if keep else []
    assert worst_engine <= 0.51, (tag, worst_engine)
    assert worst_engine <= worst_reference, (tag, worst_engine, worst_reference)
    assert worst_reference >= 2.0, (tag, worst_reference)  # the stated difference is real: the reference's chain is not an exact rounding


@pytest.mark.parametrize("tag", NATIVE16_TAGS)
def test_sampler_level_api_vs_reference_recorded_16_bit_runs(tag, dev, fused_mode):
    native16_engine_vs_reference(tag, dev)


@pytest.mark.parametrize("tag", NATIVE16_TAGS)
def test_sampler_level_api_returns_the_reference_bits(tag, dev):
    """StructuredSampler.sample on bf16 / fp16 device tensors (default mode): the reference-recorded runs of tests/golden/native16.npz --
    Euler ODE / SDE, DPM-2 SDE, DPM-3 flow, Adams-3, UniPC-3, seven steps each, every step on the reference's own inputs and its own
    history records -- come back BIT FOR BIT, `final` and the record's `prediction`, each step in one launch of skr_tape_launch."""
    from skrample_amd.sampling import native

    dt, steps, mname, sname, expr, t = native16_case(load_npz("native16.npz"), tag)
    sampler, sched, model = eval(expr, {"S": PT}), SCHEDULES[sname][1](), MODELS[mname][1]
    previous = []
    for i in range(steps):
        x, out, nz = t["x"][i].to(dev), t["out"][i].to(dev), t["noise"][i].to(dev)
        before = native.launches
        rec = sampler.sample(x, out, PT.Step.from_int(i, steps), model, sched, nz if sampler.require_noise else None, tuple(previous))
        assert native.launches == before + 1, (tag, i)
        assert rec.final.dtype == dt and torch.equal(rec.final.cpu(), t["final"][i]), (tag, i, "final")
        assert torch.equal(torch.as_tensor(rec.prediction).cpu(), t["prediction"][i]), (tag, i, "prediction")
        previous.append(rec)
        keep = sampler.require_previous
        previous = previous[max(len(previous) - keep, 0) :] if keep else []


@pytest.mark.parametrize("tag", NATIVE16_TAGS)
def test_remembered_steps_bind_new_tensors_to_the_recorded_tape(tag, dev):
    """native._remembered_step: the second run of a configuration records nothing -- every step binds its tensors to the skr_tape of the first run --
    and returns the reference's bits again; fresh tensor objects, an equal-but-distinct sampler / schedule / model; an argument pattern the first run
    did not have (one tensor given as sample AND noise) is recorded on its own"""
    from skrample_amd.sampling import native

    dt, steps, mname, sname, expr, t = native16_case(load_npz("native16.npz"), tag)
    native._remembered.clear()
    for lap in range(2):
        sampler, sched, model = eval(expr, {"S": PT}), SCHEDULES[sname][1](), MODELS[mname][1]
        previous = []
        hits = native.remembered_hits
        for i in range(steps):
            x, out, nz = t["x"][i].to(dev), t["out"][i].to(dev), t["noise"][i].to(dev)
            rec = sampler.sample(x, out, PT.Step.from_int(i, steps), model, sched, nz if sampler.require_noise else None, tuple(previous))
            assert torch.equal(rec.final.cpu(), t["final"][i]) and torch.equal(torch.as_tensor(rec.prediction).cpu(), t["prediction"][i]), (tag, lap, i)
            previous.append(rec)
            keep = sampler.require_previous
            previous = previous[max(len(previous) - keep, 0) :] if keep else []
        assert native.remembered_hits - hits == (steps if lap else 0), (tag, lap)
    if sampler.require_noise:  # the sample given as the noise too: another tape (one leaf fewer), not the remembered one
        x, out = t["x"][0].to(dev), t["out"][0].to(dev)
        hits = native.remembered_hits
        got = sampler.sample(x, out, PT.Step.from_int(0, steps), model, sched, x, ()).final.cpu()
        want = sampler.sample(x.cpu(), out.cpu(), PT.Step.from_int(0, steps), model, sched, x.cpu(), ()).final
        assert native.remembered_hits == hits and torch.equal(got, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["euler_sde", "dpm3_sde", "adams9", "unip4_sde", "unipc3_sde", "unipc2_adams3", "unipc3_deriv_flow_sde", "unipc3_noderiv"])
def test_tape_kernel_equals_the_oracles_native_chain(name, dtype, dev):
    """Every op of the tape kernel on ragged sizes: sampler families x models x schedules on device tensors whose element count is not
    a multiple of the lane width, against the oracle's reference-order chain in the tensor dtype (fp32 / fp64: native.mode = 'always')."""
    from skrample_amd.sampling import native

    mk_o, mk_p = SAMPLERS[name]
    steps, shape = 8, (3, 5, 7, 3)  # 315 elements: a ragged tail
    before, native.mode = native.mode, "always"
    try:
        for sname, mname in (("karras_scaled", "eps"), ("linear", "flow"), ("scaled", "scalex")):
            g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{sname}/{mname}/{dtype}".encode()))
            cfg, sampler = mk_o(), mk_p()
            sched, osched, (omodel, model) = SCHEDULES[sname][1](), SCHEDULES[sname][0](), MODELS[mname]
            x = torch.randn(shape, generator=g).to(dtype)
            previous, oprevious = [], []
            for i in range(steps):
                out = torch.randn(shape, generator=g).to(dtype)
                nz = torch.randn(shape, generator=g).to(dtype)
                launched = native.launches
                rec = sampler.sample(x.to(dev), out.to(dev), PT.Step.from_int(i, steps), model, sched, nz.to(dev) if sampler.require_noise else None, tuple(previous))
                assert native.launches == launched + 1
                ref = OA.sample(cfg, x, out, (i / steps, (i + 1) / steps), omodel, osched, nz if sampler.require_noise else None, oprevious)
                assert rec.final.dtype == dtype and torch.equal(rec.final.cpu(), ref.final), (name, sname, mname, i, (rec.final.cpu().double() - ref.final.double()).abs().max())
                previous.append(rec)
                oprevious.append(ref)
                keep = sampler.require_previous
                previous = previous[max(len(previous) - keep, 0) :] if keep else []
                oprevious = oprevious[max(len(oprevious) - keep, 0) :] if keep else []
                x = ref.final
    finally:
        native.mode = before


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
def test_tape_ops_through_the_c_abi(dtype, dev):
    "every op code of skr_tape_launch against the same torch op on CPU tensors of that dtype (one rounding per op), whole vectors and a ragged tail"
    lib = _hip.load()
    for numel in (4096, 1023, 3):
        g = torch.Generator().manual_seed(numel)
        a, b = torch.randn(numel, generator=g).to(dtype), (torch.randn(numel, generator=g) + 3.0).to(dtype)
        wide = torch.float64 if dtype == torch.float64 else torch.float32  # the op-math type
        T = _hip
        programs = [
            ([(T.TAPE_LOAD, 0, 0, 0, 0.0), (T.TAPE_LOAD, 1, 1, 0, 0.0), (T.TAPE_RSUB_S, 2, 0, 0, 1.5), (T.TAPE_STORE, 0, 2, 0, 0.0), (T.TAPE_RDIV_S, 2, 1, 0, 2.25), (T.TAPE_STORE, 0, 2, 1, 0.0),
              (T.TAPE_MUL, 2, 0, 1, 0.0), (T.TAPE_STORE, 0, 2, 2, 0.0), (T.TAPE_DIV, 3, 0, 1, 0.0), (T.TAPE_STORE, 0, 3, 3, 0.0)],
             lambda: [1.5 - a, (torch.tensor(2.25, dtype=wide) / b.to(wide)).to(dtype), a * b, a / b]),  # (k / x: ONE correctly rounded division; torch's own `k / tensor` is reciprocal() * k)
            ([(T.TAPE_LOAD, 5, 0, 0, 0.0), (T.TAPE_LOAD, 15, 1, 0, 0.0), (T.TAPE_NEG, 0, 5, 0, 0.0), (T.TAPE_STORE, 0, 0, 0, 0.0), (T.TAPE_MUL_S, 1, 5, 0, 0.3), (T.TAPE_ADD, 1, 1, 15, 0.0),
              (T.TAPE_DIV_S, 1, 1, 0, 0.7), (T.TAPE_ADD_S, 1, 1, 0, -0.125), (T.TAPE_SUB, 1, 1, 5, 0.0), (T.TAPE_STORE, 0, 1, 1, 0.0)],
             lambda: [-a, ((a * 0.3 + b) / 0.7 + -0.125) - a]),
            # scalars a 16-bit dtype cannot hold: torch's add / rsub round them to the tensor dtype first, its mul / div do not
            ([(T.TAPE_LOAD, 3, 0, 0, 0.0), (T.TAPE_LOAD, 4, 1, 0, 0.0), (T.TAPE_ADD_S, 0, 3, 0, 7.7), (T.TAPE_STORE, 0, 0, 0, 0.0), (T.TAPE_RSUB_S, 1, 4, 0, 0.001), (T.TAPE_STORE, 0, 1, 1, 0.0),
              (T.TAPE_MUL_S, 2, 3, 0, 7.7), (T.TAPE_STORE, 0, 2, 2, 0.0), (T.TAPE_ADD_S, 2, 4, 0, -3.3), (T.TAPE_STORE, 0, 2, 3, 0.0)],
             lambda: [a + 7.7, 0.001 - b, a * 7.7, b - 3.3]),
            # the two-op forms: a product by a scalar inside the sum / difference that reads it, rounded on its way as the op it stands for
            ([(T.TAPE_LOAD, 0, 0, 0, 0.0), (T.TAPE_LOAD, 1, 1, 0, 0.0), (T.TAPE_ADD_MS, 2, 0, 1, 0.3), (T.TAPE_STORE, 0, 2, 0, 0.0), (T.TAPE_SUB_MS, 2, 0, 1, 7.7), (T.TAPE_STORE, 0, 2, 1, 0.0),
              (T.TAPE_RSUB_MS, 3, 0, 1, -1.7), (T.TAPE_STORE, 0, 3, 2, 0.0), (T.TAPE_MULZ_S, 3, 0, 0, 0.0), (T.TAPE_STORE, 0, 3, 3, 0.0)],
             lambda: [a + b * 0.3, a - b * 7.7, b * -1.7 - a, 0 + a * 0.0]),  # (the last: -0 products come out +0, `0 + x`)
        ]
        for ops, ref in programs:
            want = ref()
            tape = _hip.TapeC()
            for j, (code, dst, ra, rb, k) in enumerate(ops):
                tape.ops[j].code, tape.ops[j].dst, tape.ops[j].a, tape.ops[j].b, tape.ops[j].k = code, dst, ra, rb, k
            tape.n_ops, tape.n_inputs, tape.n_outputs, tape.dtype = len(ops), 2, len(want), _hip.DTYPE_CODE[dtype]
            ad, bd = a.to(dev), b.to(dev)
            outs = [torch.empty(numel, dtype=dtype, device=dev) for _ in want]
            ins = (ctypes.c_void_p * 2)(ad.data_ptr(), bd.data_ptr())
            ous = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            assert lib.skr_tape_launch(ctypes.byref(tape), ins, ous, numel, _hip.current_stream_ptr(dev)) == 0
            bits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]  # (bit patterns: the sign of a zero counts)
            for got, w in zip(outs, want):
                assert torch.equal(got.cpu().view(bits), w.view(bits)), (dtype, numel, (got.cpu().double() - w.double()).abs().max())
    bad = _hip.TapeC()
    bad.n_ops, bad.n_inputs, bad.n_outputs, bad.dtype = 1, 1, 1, _hip.BF16
    bad.ops[0].code, bad.ops[0].dst, bad.ops[0].a = _hip.TAPE_MUL_S, 16, 0  # register out of range
    x = torch.zeros(8, dtype=torch.bfloat16, device=dev)
    one = (ctypes.c_void_p * 1)(x.data_ptr())
    assert lib.skr_tape_launch(ctypes.byref(bad), one, one, 8, _hip.current_stream_ptr(dev)) == 3  # SKR_ERR_TERMS
    bad.ops[0].code, bad.ops[0].dst, bad.ops[0].a, bad.ops[0].b = _hip.TAPE_ADD_MS, 0, 0, 16  # second register of a two-op form out of range
    assert lib.skr_tape_launch(ctypes.byref(bad), one, one, 8, _hip.current_stream_ptr(dev)) == 3
    bad.ops[0].code, bad.ops[0].b = 16, 0  # no such op code
    assert lib.skr_tape_launch(ctypes.byref(bad), one, one, 8, _hip.current_stream_ptr(dev)) != 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_add_noise_on_the_device_returns_the_reference_bits(dtype, dev):
    "scheduler.add_noise / scale_noise / Point.remove_noise on 16-bit device tensors: one tape launch each, the reference's three rounded ops (common.py:32-40)"
    from skrample_amd.common import Point
    from skrample_amd.sampling import native

    g = torch.Generator().manual_seed(19)
    x, n = torch.randn(3, 4, 33, 17, generator=g).to(dtype), torch.randn(3, 4, 33, 17, generator=g).to(dtype)
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    w.set_timesteps(7)
    _, sigma, alpha = w.schedule_np[3]
    before = native.launches
    got = w.add_noise(x.to(dev), n.to(dev), w.timesteps[3:4])
    assert native.launches == before + 1 and got.is_cuda and torch.equal(got.cpu(), x * float(alpha) + n * float(sigma))
    pt = Point(613.0, 0.7391, 0.6733)
    assert torch.equal(pt.remove_noise(x.to(dev), n.to(dev)).cpu(), (x - n * pt.sigma) / pt.alpha)
    zero = Point(1000.0, 1.0, 0.0)
    a, b = zero.remove_noise(x.float().to(dev), n.float().to(dev)).cpu(), (x.float() - n.float() * 1.0) / 0.0
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.fixture
def tape_words():
    "skr_tape_launch with one / two words per lane (by default a matter of tensor size), restored afterwards"
    lib = _hip.load()

    def choose(n: int) -> None:
        _hip.check(lib.skr_set_tuning(b"tape_words", n), "skr_set_tuning")

    yield choose
    choose(0)


@pytest.mark.parametrize("words", [1, 2])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64])
def test_random_tapes_equal_the_host_interpreter(dtype, words, dev, tape_words):
    """fuzz of skr_tape_launch: random straight-line tapes (every op code, scattered register numbers, values read several times and never,
    up to the register and op limits) through native._run on the device against native._run_host -- one torch op per entry on CPU tensors,
    which is the reference's own sequence of calls -- bit for bit, non-finite values included; whole vectors and ragged tails; both launch
    forms (one and two words per lane)"""
    import random

    from skrample_amd.sampling import native

    tape_words(words)
    T = _hip
    binary = (T.TAPE_ADD, T.TAPE_SUB, T.TAPE_MUL, T.TAPE_DIV)
    scalar = (T.TAPE_MUL_S, T.TAPE_DIV_S, T.TAPE_ADD_S, T.TAPE_RSUB_S)
    for seed in range(24):
        rng = random.Random(seed * 7 + 1)
        numel = rng.choice((8192, 4096 + 5, 1023, 37, 8, 3, 3 * 4096 + 11))
        g = torch.Generator().manual_seed(seed)
        n_leaves = rng.randint(1, 6)
        leaves = [(torch.randn(numel, generator=g) * rng.choice((0.1, 1.0, 30.0)) + rng.choice((0.0, 2.0))).to(dtype) for _ in range(n_leaves)]
        tapes = []
        for device in ("cpu", dev):
            tape = native.Tape(dtype, (numel,), torch.device(device), require_device=False)
            vals = [tape.leaf(t.to(device)) for t in leaves]
            r2 = random.Random(seed)  # the same program on both sides
            for _ in range(r2.randint(3, 40)):
                live = vals[-8:] if r2.random() < 0.7 else vals  # mostly recent values, sometimes an old one (long live ranges)
                a = r2.choice(live)
                kind = r2.random()
                if kind < 0.45:
                    code, b = r2.choice(binary), r2.choice(live)
                    v = {T.TAPE_ADD: a + b, T.TAPE_SUB: a - b, T.TAPE_MUL: a * b, T.TAPE_DIV: a / b}[code]
                elif kind < 0.9:
                    k = r2.choice((0.5, -1.25, 3.0, 0.1, 1e-3, 7.7, 1.0))
                    v = {T.TAPE_MUL_S: lambda: a * k, T.TAPE_DIV_S: lambda: a / k, T.TAPE_ADD_S: lambda: a + k, T.TAPE_RSUB_S: lambda: k - a}[r2.choice(scalar)]()
                elif kind < 0.95:
                    v = -a
                else:
                    v = r2.choice((2.0, -0.5, 7.7)) / a  # reciprocal() * k, as torch's k / tensor
                vals.append(v)
            results = r2.sample(vals[n_leaves:], min(len(vals) - n_leaves, r2.randint(1, 4)))
            tapes.append((tape, results))
        try:
            host = native._run_host(*tapes[0])
            card = native._run(*tapes[1])
        except native._Refused:
            continue  # (more live values than registers, or more ops than a tape holds: the caller would take the fused path)
        for h, c in zip(host, card):
            c = c.cpu()
            assert c.dtype == dtype and torch.equal(torch.isnan(h), torch.isnan(c)), (seed, dtype)
            assert torch.equal(torch.nan_to_num(h, nan=0.0), torch.nan_to_num(c, nan=0.0)), (seed, dtype, numel, (h.double() - c.double()).abs().max())


@pytest.mark.parametrize("seed", range(48))
def test_random_linear_forms_vs_float64(seed, dev):
    """fuzz of the fused evaluator (lazy.evaluate -> skr_step_launch): one or two random linear forms over 1-18 tensors of mixed dtypes (a narrow
    group, a wide group, stragglers of a third dtype), zero and negative coefficients, an optional chained second output, ragged sizes -- against
    the same sums in float64 on the CPU, within the accumulation error of the kernel's accumulator plus one rounding of the output dtype"""
    import random

    rng = random.Random(9000 + seed)
    numel = rng.choice((4096, 2048 * 3, 1000, 37, 8 * 511 + 3, 5))
    narrow = rng.choice((torch.bfloat16, torch.float16, torch.float32))
    wide = rng.choice((torch.float32, torch.float64)) if narrow != torch.float32 else rng.choice((torch.float32, torch.float64))
    third = rng.choice((torch.bfloat16, torch.float16, torch.float32))
    g = torch.Generator().manual_seed(seed)
    n_terms = rng.randint(1, 18)
    tensors, coefs0, coefs1 = [], [], []
    for _ in range(n_terms):
        dt = rng.choices((narrow, wide, third), weights=(6, 3, 1))[0]
        tensors.append((torch.randn(numel, generator=g) * rng.choice((0.05, 1.0, 20.0))).to(dt))
        coefs0.append(rng.choice((0.0, 1.0, -1.0, rng.uniform(-3, 3), rng.uniform(-1e-3, 1e-3))))
        coefs1.append(rng.choice((0.0, 0.0, 1.0, rng.uniform(-3, 3))))
    if all(c == 0.0 for c in coefs0):
        coefs0[0] = 1.0
    two = rng.random() < 0.5
    chain = rng.choice((0.0, 1.0, -0.75)) if two else 0.0
    acc64 = wide == torch.float64
    out_dtypes = [rng.choice((narrow, wide)), rng.choice((narrow, wide))]
    on_card = [t.to(dev) for t in tensors]
    f0 = None
    for t, c in zip(on_card, coefs0):
        term = lazy.Lin.leaf(t) * c
        f0 = term if f0 is None else f0 + term
    forms = [f0]
    if two:
        f1 = f0.node() * chain if chain != 0.0 else None
        for t, c in zip(on_card, coefs1):
            if c != 0.0:
                term = lazy.Lin.leaf(t) * c
                f1 = term if f1 is None else f1 + term
        if f1 is None:
            f1 = lazy.Lin.leaf(on_card[0]) * 1.0
            coefs1[0] = 1.0
        forms.append(f1)
    try:
        got = lazy.evaluate(forms, out_dtypes[: len(forms)])
    except _hip.SkrampleHipError as exc:
        assert "exceed the kernel limit" in str(exc) or "incompatible" in str(exc), exc  # (stated refusals: too many operands, an output dtype outside the two groups)
        return
    wide64 = [t.double() for t in tensors]
    acc0 = sum(c * t for c, t in zip(coefs0, wide64))
    mag0 = sum(abs(c) * t.abs() for c, t in zip(coefs0, wide64))
    refs, mags = [acc0], [mag0]
    if two:
        refs.append(chain * acc0 + sum(c * t for c, t in zip(coefs1, wide64)))
        mags.append(abs(chain) * mag0 + sum(abs(c) * t.abs() for c, t in zip(coefs1, wide64)))
    eps_acc = 2.0**-52 if acc64 else 2.0**-23
    for out, ref, mag, od in zip(got, refs, mags, out_dtypes):
        assert out.dtype == od and out.is_cuda
        eps_out = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24, torch.float64: 2.0**-53}[od]
        allowed = (n_terms + 4) * eps_acc * mag + eps_out * ref.abs() * 1.01 + 1e-30
        if od == torch.float16:
            allowed = allowed + 2.0**-25  # (subnormal halves)
        err = (out.cpu().double() - ref).abs()
        assert (err <= allowed).all(), (seed, narrow, wide, third, od, n_terms, two, chain, (err / allowed).max().item())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_model_transforms_on_the_device_return_the_reference_bits(dtype, dev):
    """DiffusionModel.to_x / from_x / forward / backward and ModelConvert.output_to called directly on 16-bit device tensors: one tape launch each, equal
    to the same call on host tensors -- which runs the reference's own torch ops (tools/sweep_vs_reference.py `model`: 3000 cases against the reference)"""
    from skrample_amd.common import DeltaPoint, Point
    from skrample_amd.sampling import native

    g = torch.Generator().manual_seed(23)
    s_, o_, n_ = (torch.randn(3, 4, 33, 17, generator=g).to(dtype) for _ in range(3))
    p0, p1 = Point(500.0, 0.6, 0.8), Point(300.0, 0.3, 0.9539392014169456)
    d = DeltaPoint(p0, p1)
    for model in (PM.NoiseModel(), PM.FlowModel(), PM.VelocityModel(), PM.ScaleX(bias=-1.5)):
        calls = {
            "to_x": lambda a, b, c: model.to_x(a, b, p0), "from_x": lambda a, b, c: model.from_x(a, b, p0), "forward": lambda a, b, c: model.forward(a, b, d, c, 0.5),
            "backward": lambda a, b, c: model.backward(a, b, d), "convert": lambda a, b, c: PM.ModelConvert(model, PM.VelocityModel()).output_to(a, b, p0),
        }  # fmt: skip
        for name, call in calls.items():
            before = native.launches
            got = call(s_.to(dev), o_.to(dev), n_.to(dev))
            assert native.launches == before + 1 and got.is_cuda and torch.equal(got.cpu(), call(s_, o_, n_)), (type(model).__name__, name)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_functional_samplers_on_16_bit_device_tensors_equal_the_host_run(dtype, dev):
    "RKUltra / DynasauRK / the structured adapter over a 16-bit device tensor: the recorded expressions of native.step_tableau give the bits of the host run (the reference's own torch ops)"
    from skrample_amd.sampling import functional as PF
    from skrample_amd.sampling import interface as PI
    from skrample_amd.sampling import native

    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 4, 16, 16, generator=g).to(dtype)
    draws = [torch.randn(2, 4, 16, 16, generator=g).to(dtype) for _ in range(40)]
    # (the network is torch's own code on either side: a product with a host-computed factor -- torch adds / subtracts a Python number to a 16-bit tensor
    #  differently on the CPU, where it rounds the number to the tensor dtype first, and on the device; and its device kernel for fp16 * number rounds once
    #  where the CPU rounds to fp32 and then to fp16 -- hence the product in explicit fp32 steps)
    net = lambda xx, t, s, a: (xx.float() * (0.3 - 0.1 * s + 0.05 * a)).to(xx.dtype)  # noqa: E731
    for sampler, model, schedule in (
        (PF.RKUltra(order=4), PM.NoiseModel(), PS.Scaled()),
        (PF.RKUltra(order=3, stochasticity=1, derivative_transform=PM.VelocityModel()), PM.FlowModel(), PS.Linear()),
        (PF.DynasauRK(order=3), PM.VelocityModel(), PS.Karras(PS.Scaled())),
        (PI.StructuredFunctionalAdapter(PT.UniPC(order=3, stochasticity=0.5)), PM.NoiseModel(), PS.Scaled()),
    ):
        pools = [list(draws), [d.to(dev) for d in draws]]
        host = sampler.sample_model(x, net, model, schedule, 5, rng=lambda *_: pools[0].pop(0))
        before = native.launches
        card = sampler.sample_model(x.to(dev), net, model, schedule, 5, rng=lambda *_: pools[1].pop(0))
        assert native.launches > before and card.is_cuda and card.dtype == dtype and torch.equal(card.cpu(), host), sampler


def test_step_programs_tell_a_runs_first_record_from_a_state(dev):
    """A history record's `sample` is the caller's tensor after the first step of a run and a state tensor (UniPC's corrected, SPC's blended sample) later;
    the lowered step programs are kept per (index, history steps, ...) and must not be replayed across that difference.  Two ways there: a schedule that
    hands out one timestep several times (Exponential over ZSNR: 1000.0 six times, every one resolving to index 0 as in the reference; found by
    tests/soak_sweep.py seed 851552), and one scheduler object used for a run from the middle of the schedule and then for a full run."""
    shape = (3, 3, 7, 8)
    g = torch.Generator().manual_seed(851552)
    for dt in (torch.float16, torch.bfloat16):
        mk = lambda: PD.SkrampleWrapperScheduler(PT.SPC(predictor=PT.Euler(stochasticity=0.5), corrector=PT.Euler(stochasticity=0.5), invert=True), PS.Exponential(PS.ZSNR()), PM.VelocityModel())  # noqa: E731
        host, card = mk(), mk()
        host.set_timesteps(8)
        card.set_timesteps(8)
        assert host.timesteps.tolist().count(host.timesteps[0].item()) > 2  # (the premise: repeated timesteps)
        x = torch.randn(shape, generator=g).to(dt)
        outs = [torch.randn(shape, generator=g).to(dt) for _ in range(8)]
        noises = [torch.randn(shape, generator=g) for _ in range(8)]
        host._noise_generator, card._noise_generator = Injected(noises, "cpu"), Injected(noises, dev)
        for i, t in enumerate(host.timesteps):
            want = host.step(outs[i], t, x, return_dict=False)[0]
            got = card.step(outs[i].to(dev), t, x.to(dev), return_dict=False)[0]
            want, got = (torch.as_tensor(v.materialize() if isinstance(v, lazy.LazyTensor) else v) for v in (want, got))
            assert_close(got, want, dt, f"repeated timesteps {dt} step {i}", flips=0.2)
            x = want
    # one scheduler object: a run over the last steps of the schedule, then a full run -- index 5 follows a first record in the one, a state in the other
    host, card = (PD.SkrampleWrapperScheduler(PT.UniPC(order=2), PS.Scaled()) for _ in range(2))
    steps, dt = 8, torch.bfloat16
    outs = [torch.randn(shape, generator=g).to(dt) for _ in range(steps)]
    x0 = torch.randn(shape, generator=g).to(dt)
    for first in (4, 0, 3):
        host.set_timesteps(steps)
        card.set_timesteps(steps)
        x = x0
        for i in range(first, steps):
            t = host.timesteps[i]
            want = host.step(outs[i], t, x, return_dict=False)[0]
            got = card.step(outs[i].to(dev), t, x.to(dev), return_dict=False)[0]
            want, got = (torch.as_tensor(v.materialize() if isinstance(v, lazy.LazyTensor) else v) for v in (want, got))
            assert_close(got, want, dt, f"run from {first}, step {i}", flips=0.2)
            x = want


def test_a_generator_of_a_third_dtype_is_cast_to_the_compute_scale(dev):
    """fp16 latents, compute_scale=float64 and a noise generator object that returns fp32 tensors: the reference casts what the generator returns to the compute
    scale (diffusers.py:346); here that used to hand the step kernel three operand dtypes (found by tests/soak_sweep.py seed 860587)"""
    shape, steps, dt = (1, 2, 8, 8), 9, torch.float16
    g = torch.Generator().manual_seed(860587)
    host, card = (PD.SkrampleWrapperScheduler(PT.UniPC(order=2, stochasticity=-1.5), PS.Beta(PS.Linear()), PM.DataModel(), compute_scale=torch.float64) for _ in range(2))
    host.set_timesteps(steps)
    card.set_timesteps(steps)
    x = torch.randn(shape, generator=g).to(dt)
    outs = [torch.randn(shape, generator=g).to(dt) for _ in range(steps)]
    noises = [torch.randn(shape, generator=g) for _ in range(steps)]
    host._noise_generator, card._noise_generator = Injected(noises, "cpu"), Injected(noises, dev)
    for i, t in enumerate(host.timesteps):
        want = host.step(outs[i], t, x, return_dict=False)[0]
        got = card.step(outs[i].to(dev), t, x.to(dev), return_dict=False)[0]
        want, got = (torch.as_tensor(v.materialize() if isinstance(v, lazy.LazyTensor) else v) for v in (want, got))
        assert_close(got, want, dt, f"step {i}", flips=0.2)
        x = want


def test_wrappers_keep_their_compute_scale(dev):
    "the scheduler wrappers widen to compute_scale before the sampler runs (reference diffusers.py:575-599): fused kernel; compute_scale=None: the tape"
    from skrample_amd.sampling import native

    shape, steps = (2, 4, 16, 16), 6
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    outs = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(steps)]

    def run(w):
        w.set_timesteps(steps)
        x = x0
        for t, o in zip(w.timesteps.tolist(), outs):
            x = w.step(o, t, x, return_dict=False)[0]
        return x

    launched = native.launches
    wide = run(PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled()))
    assert native.launches == launched  # fp32 compute scale: one fused launch per step, as ever
    narrow = run(PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled(), compute_scale=None))
    assert native.launches == launched + steps  # no widening asked for: the reference computes in bf16, and so does the tape
    assert narrow.dtype == wide.dtype == torch.bfloat16 and not torch.equal(narrow, wide)
    assert ((narrow.float() - wide.float()).abs().max() / wide.float().abs().max()).item() < 0.05  # (a 6-step bf16 chain drifts by a few last places)


@pytest.mark.parametrize("shape", [(3, 4, 32, 32), (2, 3, 16, 16), (2, 6, 16, 16), (3, 1, 8, 8)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_in_kernel_philox_matches_oracle_spec(dtype, shape, dev):
    """DPM-2 SDE with Random noise drawn inside the step kernel == oracle fed the spec'd Philox normals
    (bf16: 8 consecutive elements per lane; fp32: the whole-line tile layout -- the element -> Philox block map must hold in both)"""
    # per-sample sizes 4096 (whole tiles), 768 (launch is whole tiles, samples are not: 8-consecutive layout),
    # 1536 (three tiles per sample: partial block on the per-sample grid), 64 (flat grid)
    steps, seeds = 7, [11, 2**40 + 5, 2**63 + 9][: shape[0]]
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))
    o = OW.StepDriver(OA.make("dpm", 2, eta=1), OS.karras(OS.scaled(), steps=steps), "eps")
    w.set_timesteps(steps)
    o.set_timesteps(steps)
    g = torch.Generator().manual_seed(5)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    x = torch.randn(shape, generator=g).to(dtype)
    n = shape[1] * shape[2] * shape[3]
    for i, t in enumerate(w.timesteps):
        out = torch.randn(shape, generator=g).to(dtype)
        got = w.step(out.to(dev), t, x.to(dev), generator=gens, return_dict=False)[0]
        noise = torch.from_numpy(np.stack([ON.philox_normal(s, i * 256, n) for s in seeds])).reshape(shape)
        ref = o.step(out, t, x, noise=noise)[0]
        assert_close(got, ref, dtype, f"philox step {i}")
        x = ref


def test_unipc_sde_fused_two_draws(dev):
    "UniPC SDE: corrector re-draws the previous step's noise, predictor the current one, in one launch"
    steps, shape, seeds = 6, (2, 16, 16, 16), [3, 4]
    w = PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Linear(), PM.FlowModel())
    o = OW.StepDriver(OA.make("unipc", 3, eta=1), OS.linear(), "flow")
    w.set_timesteps(steps)
    o.set_timesteps(steps)
    g = torch.Generator().manual_seed(6)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    x = torch.randn(shape, generator=g)
    n = shape[1] * shape[2] * shape[3]
    for i, t in enumerate(w.timesteps):
        out = torch.randn(shape, generator=g)
        got = w.step(out.to(dev), t, x.to(dev), generator=gens, return_dict=False)[0]
        noise = torch.from_numpy(np.stack([ON.philox_normal(s, i * 256, n) for s in seeds])).reshape(shape)
        ref = o.step(out, t, x, noise=noise)[0]
        assert_close(got, ref, torch.float32, f"unipc philox step {i}")
        x = ref


def test_edge_shapes(dev):
    "empty batch, ragged sizes (numel % 8 != 0, sample_numel % 8 != 0 with noise), misaligned views, non-contiguous"
    sched, model = PS.Scaled(), PM.NoiseModel()
    osched = OS.scaled()
    smp = PT.Euler(stochasticity=1)
    for shape in [(0, 4, 8, 8), (1, 1, 1, 1), (3, 1, 5, 7), (2, 3, 9, 11), (1, 4, 64, 64)]:
        g = torch.Generator().manual_seed(sum(shape))
        x, out, nz = (torch.randn(shape, generator=g) for _ in range(3))
        rec = smp.sample(x.to(dev), out.to(dev), (0.2, 0.3), model, sched, nz.to(dev))
        assert tuple(rec.final.shape) == shape
        if x.numel():
            ref = OA.sample(OA.make("euler", eta=1), x, out, (0.2, 0.3), "eps", osched, nz).final
            assert_close(rec.final, ref, torch.float32, str(shape))
    # ragged sample size with in-kernel-style noise: falls back to skr_noise_random + ordinary term
    shape, seeds = (3, 1, 5, 7), [9, 8, 7]
    pn = lazy.PhiloxNoise(torch.tensor(seeds, dtype=torch.int64, device=dev), 512, shape, dev)
    assert not pn.fusable()
    g = torch.Generator().manual_seed(1)
    x, out = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    rec = smp.sample(x.to(dev), out.to(dev), (0.2, 0.3), model, sched, pn)
    noise = torch.from_numpy(np.stack([ON.philox_normal(s, 512, 35) for s in seeds])).reshape(shape)
    assert_close(rec.final, OA.sample(OA.make("euler", eta=1), x, out, (0.2, 0.3), "eps", osched, noise).final, torch.float32, "ragged philox")
    # misaligned + non-contiguous operands are normalised, never mis-read
    base = torch.randn(2 * 4 * 16 * 16 + 3, generator=g).to(dev)
    xv = base[3:].view(2, 4, 16, 16)
    ov = torch.randn(2, 16, 16, 4, generator=g).to(dev).permute(0, 3, 1, 2)
    rec = PT.Euler().sample(xv, ov, (0.2, 0.3), model, sched)
    ref = OA.sample(OA.make("euler"), xv.cpu(), ov.cpu().contiguous(), (0.2, 0.3), "eps", osched).final
    assert_close(rec.final, ref, torch.float32, "views")


def test_c_abi_direct(dev):
    "call skr_step_launch by hand: two dtype groups, two outputs with chain, status codes"
    lib = _hip.load()
    n = 4 * 1024 + 5
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(n, generator=g).bfloat16().to(dev), torch.randn(n, generator=g).bfloat16().to(dev)
    c = torch.randn(n, generator=g).to(dev)
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b = 3, 2, _hip.BF16, _hip.F32
    plan.out0_dtype, plan.out1_dtype, plan.chain = _hip.F32, _hip.BF16, 0.75
    for k, (c0, c1) in enumerate([(1.5, 0.0), (-0.25, 2.0), (0.5, -1.0)]):
        plan.coef0[k], plan.coef1[k] = c0, c1
    o0, o1 = torch.empty(n, device=dev), torch.empty(n, device=dev, dtype=torch.bfloat16)
    _hip.launch_step(plan, [a, b, c], o0, o1, None, n, dev)
    r0 = 1.5 * a.float() - 0.25 * b.float() + 0.5 * c
    r1 = 0.75 * r0 + 2.0 * b.float() - c
    assert_close(o0, r0, torch.float32, "out0")
    assert_close(o1, r1.bfloat16(), torch.bfloat16, "out1")
    plan.dtype_a = 7
    ptrs = (ctypes.c_void_p * 3)(a.data_ptr(), b.data_ptr(), c.data_ptr())
    assert lib.skr_step_launch(ctypes.byref(plan), ptrs, o0.data_ptr(), o1.data_ptr(), None, n, None) == 2  # SKR_ERR_DTYPE
    plan.dtype_a, plan.noise_mode, plan.zeta0, plan.sample_numel = _hip.BF16, 1, 1.0, 7
    assert lib.skr_step_launch(ctypes.byref(plan), ptrs, o0.data_ptr(), o1.data_ptr(), None, n, None) == 1  # seeds missing
    seeds = torch.zeros(1, dtype=torch.int64, device=dev)
    assert lib.skr_step_launch(ctypes.byref(plan), ptrs, o0.data_ptr(), o1.data_ptr(), seeds.data_ptr(), n, None) == 5  # numel % sample_numel
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize(("kinds", "n_terms"), [((1, 0), 2), ((1, 1), 4), ((2, 2), 7), ((3, 3), 8), ((0, 1), 5)])
def test_runge_kutta_stage_kernels_agree_bitwise(dtype, kinds, n_terms, dev):
    """the compile-time-K stage kernel (numel % 8 == 0) and the general kernel (ragged numel, same leading data)
    must produce the same derivative and the same next stage input, bit for bit"""
    n = 8 * 1024
    g = torch.Generator().manual_seed(n_terms)
    ins_long = [torch.randn(n + 3, generator=g).to(dtype).to(dev) for _ in range(n_terms)]
    ins_short = [t[:n].clone() for t in ins_long]
    plan = _hip.StepPlanC()
    code = _hip.DTYPE_CODE[dtype]
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b = n_terms, n_terms, code, code
    plan.out0_dtype, plan.out1_dtype, plan.chain = code, code, 0.3125
    plan.convert_to, plan.convert_from = kinds
    for i, v in enumerate((0.7, 0.9, 0.4, 1.3)):
        plan.convert_k[i] = v
    for k in range(n_terms):
        plan.coef0[k], plan.coef1[k] = 0.0, (-1) ** k * (0.2 + 0.1 * k)
    outs = []
    for ins, m in ((ins_short, n), (ins_long, n + 3)):
        o0, o1 = torch.full((m,), 7.0, device=dev, dtype=dtype), torch.full((m,), 7.0, device=dev, dtype=dtype)
        _hip.launch_step(plan, ins, o0, o1, None, m, dev)
        outs.append((o0, o1))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0][:n]) and torch.equal(outs[0][1], outs[1][1][:n])
    assert torch.isfinite(outs[0][0].float()).all() and outs[0][0].float().abs().max() > 0.1


@pytest.mark.parametrize(("dtypes", "n_terms", "two_outputs"), [((torch.float32, torch.float32), 1, False), ((torch.float32, torch.float32), 4, False), ((torch.float32, torch.float32), 8, False),
                                                                  ((torch.float32, torch.float32), 11, True), ((torch.bfloat16, torch.float32), 6, True), ((torch.float16, torch.float32), 9, True), ((torch.bfloat16, torch.float32), 3, False)])
def test_tile_layout_agrees_bitwise(dtypes, n_terms, two_outputs, dev):
    """launches made of whole 512-element tiles use the whole-line tile layout when a 32-bit tensor takes part; a ragged
    launch over the same leading data uses 8 consecutive elements per lane -- same bits required"""
    ta, tb = dtypes
    n = 512 * 37
    g = torch.Generator().manual_seed(n_terms)
    n_a = n_terms if ta == tb else max(1, n_terms // 2)
    long_ins = [torch.randn(n + 5, generator=g).to(ta if k < n_a else tb).to(dev) for k in range(n_terms)]
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b = n_terms, n_a, _hip.DTYPE_CODE[ta], _hip.DTYPE_CODE[tb]
    plan.out0_dtype = _hip.F32
    plan.out1_dtype = _hip.DTYPE_CODE[ta] if two_outputs else -1
    plan.chain = -0.375
    for k in range(n_terms):
        plan.coef0[k], plan.coef1[k] = (-1) ** k * (0.3 + 0.05 * k), 0.1 * (k + 1)
    res = []
    for m in (n, n + 5):
        ins = [t[:m].clone() for t in long_ins]
        o0 = torch.full((m,), 3.0, device=dev)
        o1 = torch.full((m,), 3.0, device=dev, dtype=ta) if two_outputs else None
        _hip.launch_step(plan, ins, o0, o1, None, m, dev)
        res.append((o0, o1))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0][:n])
    if two_outputs:
        assert torch.equal(res[0][1], res[1][1][:n])
    ref = sum(plan.coef0[k] * long_ins[k][:n].double() for k in range(n_terms))
    assert rel_err(res[0][0], ref) < 1e-5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize(
    ("n_terms", "noise", "rk"),
    [(1, False, False), (4, True, False), (4, False, False), (8, True, False), (2, False, True), (5, False, True), (8, False, True), (3, True, True), (6, True, True)]
    # round 3: compile-time kernels up to 20 operands (Adams-Bashforth 5-9: 10-18 operands; the `one_trip` switch sends these to the general kernel)
    + [(9, False, False), (10, False, False), (12, True, False), (13, False, False), (14, False, False), (16, True, False), (17, False, False), (18, False, False), (20, True, False)],
)
@pytest.mark.parametrize("chunks_per_sample", [64, 18])
def test_one_trip_kernels_agree_bitwise(dtype, n_terms, noise, rk, chunks_per_sample, dev):
    """launches made of whole 2048-element chunks take the one-trip loads-first kernels (XCD-aware chunk map, 1-D grid);
    the grid-stride kernels they replace (still used for ragged shapes) and the identity chunk map must give the same bits,
    including the in-kernel Philox draws (same block numbering per sample)."""
    lib = _hip.load()
    # 64 chunks per sample (a power of two: shift) or 18 (4x96x96 latents: the kernel divides); 384 / 108 chunks in all
    batch, sample = 6, 2048 * chunks_per_sample
    n = batch * sample
    g = torch.Generator().manual_seed(100 * n_terms + noise)
    ins = [torch.randn(n, generator=g).to(dtype).to(dev) for _ in range(n_terms)]
    seeds = torch.arange(batch, dtype=torch.int64, device=dev) * 7919 + 3
    code = _hip.DTYPE_CODE[dtype]
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.out0_dtype = n_terms, n_terms, code, code, code
    plan.out1_dtype = code if rk else -1
    plan.sample_numel = sample
    for k in range(n_terms):
        plan.coef0[k], plan.coef1[k] = (-1) ** k * (0.3 + 0.05 * k), 0.1 * (k + 1) - 0.35
    if noise:
        plan.noise_mode, plan.zeta0, plan.stream0 = 1, 0.625, 11
    if rk:
        if noise:  # the stochastic last stage: the draw lands on out1, the derivative (out0) stays clean
            plan.zeta0, plan.zeta1, plan.stream1 = 0.0, 0.625, 11
        plan.convert_to, plan.convert_from, plan.chain = 1, 2, 0.3125
        for i, v in enumerate((0.7, 0.9, 0.4, 1.3)):
            plan.convert_k[i] = v
    results = []
    try:
        for one_trip, xmap in ((1, 3), (1, 0), (1, 1), (0, 0)):
            assert lib.skr_set_tuning(b"one_trip", one_trip) == 0 and lib.skr_set_tuning(b"xmap", xmap) == 0
            o0 = torch.full((n,), 5.0, device=dev, dtype=dtype)
            o1 = torch.full((n,), 5.0, device=dev, dtype=dtype) if rk else None
            _hip.launch_step(plan, ins, o0, o1, seeds if noise else None, n, dev)
            torch.cuda.synchronize()
            results.append((o0, o1))
    finally:
        lib.skr_set_tuning(b"reset", 0)
    for o0, o1 in results[1:]:
        assert torch.equal(o0, results[0][0])
        if rk:
            assert torch.equal(o1, results[0][1])
    out = results[0][1] if rk else results[0][0]
    assert torch.isfinite(out.float()).all() and out.float().std() > 0.1
    assert lib.skr_set_tuning(b"no_such_switch", 1) == 7  # SKR_ERR_UNSUPPORTED


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize(
    ("n_a", "n_b", "noise"),
    [(2, 0, True), (3, 0, False), (4, 0, True), (4, 1, True), (6, 1, False), (7, 1, False), (8, 1, True), (10, 1, False), (8, 1, False)]
    + [(12, 1, True), (14, 1, False), (16, 1, True), (18, 1, False), (20, 1, True), (22, 1, False)],  # round 3: UniPC / SPC of order 5-9
)
def test_two_output_kernels_agree_bitwise(dtype, n_a, n_b, noise, dev):
    """UniPC / SPC steps (fp32 state out0 + 16-bit out1, 16-bit operands + at most one fp32 state) take a compile-time
    one-trip kernel when the launch is made of whole chunks; it must give the bits of the general runtime-term-list kernel,
    both Philox draws (two streams) included -- and a zero zeta must leave -0.0 sums alone exactly as the general kernel does."""
    lib = _hip.load()
    batch, sample = 3, 2048 * 16
    n = batch * sample
    g = torch.Generator().manual_seed(10 * n_a + n_b)
    ins = [torch.randn(n, generator=g).to(dtype).to(dev) for _ in range(n_a)] + [torch.randn(n, generator=g).to(dev) for _ in range(n_b)]
    ins[0][:64] = 0  # exact zeros in, so some sums are signed zeros
    seeds = torch.arange(batch, dtype=torch.int64, device=dev) * 104729 + 17
    code = _hip.DTYPE_CODE[dtype]
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b = n_a + n_b, n_a, code, _hip.F32
    plan.out0_dtype, plan.out1_dtype, plan.chain, plan.sample_numel = _hip.F32, code, -0.4375, sample
    for k in range(n_a + n_b):
        plan.coef0[k], plan.coef1[k] = (-1) ** k * (0.25 + 0.05 * k), 0.3 - 0.07 * k
    variants = [(0.0, 0.0)]
    if noise:
        plan.noise_mode, plan.stream0, plan.stream1 = 1, 5, 6
        variants = [(0.5, 0.75), (0.0, 0.75), (0.5, 0.0)]
    try:
        for z0, z1 in variants:
            plan.zeta0, plan.zeta1 = z0, z1
            res = []
            for fast in (2, 0):  # 2 = take the compile-time kernel for every shape it is instantiated for
                assert lib.skr_set_tuning(b"two_out", fast) == 0
                o0 = torch.full((n,), 9.0, device=dev)
                o1 = torch.full((n,), 9.0, device=dev, dtype=dtype)
                _hip.launch_step(plan, ins, o0, o1, seeds if noise else None, n, dev)
                torch.cuda.synchronize()
                res.append((o0, o1))
            assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)), (z0, z1)
            assert torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16)), (z0, z1)
            assert torch.isfinite(res[0][0]).all() and res[0][0].std() > 0.1
    finally:
        lib.skr_set_tuning(b"reset", 0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("kinds", [(1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 2), (3, 3), (1, 2)])
def test_rounded_conversion_equals_torch_op_by_op(dtype, kinds, dev):
    """the RK wrapper's derivative (out0 of a CONV launch) must carry exactly the roundings torch applies when the
    reference evaluates to_x / from_x one tensor op at a time in the input dtype (fp32 op result, then the tensor
    dtype: in fp16 a fused multiply-convert would round once and miss the reference on fp32 ties)"""
    n = 8 * 4096
    g = torch.Generator().manual_seed(zlib.crc32(repr(kinds).encode()) % 1000)
    s_, o_ = (torch.randn(n, generator=g) * 1.5).to(dtype), torch.randn(n, generator=g).to(dtype)
    k = (0.9, 0.09999999999999998, 0.7310585786300049, 0.35)
    to_kind, from_kind = kinds
    x = {0: lambda: o_, 1: lambda: (s_ - k[0] * o_) / k[1], 2: lambda: k[1] * s_ - k[0] * o_, 3: lambda: o_ * k[0]}[to_kind]()
    ref = {0: lambda: x, 1: lambda: (s_ - k[2] * x) / k[3], 2: lambda: (k[2] * s_ - x) / k[3], 3: lambda: x / k[2]}[from_kind]()
    assert ref.dtype == dtype
    plan = _hip.StepPlanC()
    code = _hip.DTYPE_CODE[dtype]
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b = 2, 2, code, code
    plan.out0_dtype, plan.out1_dtype, plan.chain = code, code, 1.0
    plan.convert_to, plan.convert_from = kinds
    for i, v in enumerate(k):
        plan.convert_k[i] = v
    for m in (n, n - 3):  # compile-time-K stage kernel, general kernel
        o0, o1 = torch.empty(m, device=dev, dtype=dtype), torch.empty(m, device=dev, dtype=dtype)
        _hip.launch_step(plan, [s_[:m].clone().to(dev), o_[:m].clone().to(dev)], o0, o1, None, m, dev)
        torch.cuda.synchronize()
        assert torch.equal(o0.cpu(), ref[:m]), (dtype, kinds, m, int((o0.cpu() != ref[:m]).sum()))


def test_wrapper_contract(dev):
    "return types, dtype/device of results, ValueError on unknown timestep, history trimming, no sync for device timesteps"
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=3), PS.Scaled())
    w.set_timesteps(5, device=dev)
    assert w.timesteps.device.type == "cuda" and len(w.sigmas) == 6 and w.init_noise_sigma == 1 and w.order == 1
    x = torch.randn(1, 4, 8, 8, device=dev).bfloat16()
    for t in w.timesteps:  # device-resident timesteps: consumed in order without .item()
        res = w.step(torch.randn_like(x), t, x)
        assert res.prev_sample.dtype == torch.bfloat16 and res.prev_sample.device == x.device and res["prev_sample"] is res.prev_sample
        x = res.prev_sample
    assert len(w._previous) == 2
    w.set_timesteps(5)
    with pytest.raises(ValueError):
        w.step(x, 123.456, x)
    assert torch.equal(w.scale_model_input(x, w.timesteps[0]), x)
    noisy = w.add_noise(x, torch.randn_like(x), w.timesteps[1:2])
    assert noisy.shape == x.shape and noisy.dtype == x.dtype
    r = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=2)
    r.set_timesteps(3)
    with pytest.raises(AssertionError):
        r.step(x, 1.0, x)


def test_diffusers_inverse(dev):
    "reference test_diffusers_inverse: invert_prediction on a negated network == forward, bit-exact"
    weights = torch.randn(64, 64, dtype=torch.float32, device=dev) * 0.1
    net = lambda x, t: x @ weights + x * (float(t) / 1000)  # noqa: E731
    for cls in (PD.SkrampleWrapperScheduler, PD.RKUltraWrapperScheduler, PD.DynasauRKWrapperScheduler):
        fwd = cls.from_diffusers_config({"shift": 12})
        bwd = cls.from_diffusers_config({"shift": 12}, invert_prediction=True)
        x0 = torch.randn(64, 64, device=dev)
        a, b = x0.clone(), x0.clone()
        fwd.set_timesteps(num_inference_steps=10)
        bwd.set_timesteps(num_inference_steps=10)
        for t in fwd.timesteps:
            a = fwd.step(net(a, t), t, a, return_dict=False)[0]
        for t in bwd.timesteps:
            b = bwd.step(-net(b, t), t, b, return_dict=False)[0]
        assert torch.equal(a, b), cls.__name__


def test_functional_samplers_on_device(dev):
    "RKUltra / adapter loops with a closure model on HIP tensors vs the oracle"
    sched_p, sched_o = PS.Scaled(), OS.scaled()
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 4, 16, 16, generator=g)
    wmat = torch.randn(16, 16, generator=g) * 0.05
    model_cpu = lambda x, t, s, a: x @ wmat + x * s  # noqa: E731
    wdev = wmat.to(dev)
    model_dev = lambda x, t, s, a: x @ wdev + x * s  # noqa: E731
    from skrample_amd.sampling import functional as PF
    from skrample_amd.sampling import interface as PI

    for order in (2, 4, 6):
        got = PF.RKUltra(order=order).sample_model(x0.to(dev), model_dev, PM.VelocityModel(), sched_p, 4)
        ref = OK.rk_loop(lambda st: OK.pick_tableau(order), x0, model_cpu, "v", sched_o, 4)
        assert_close(got, ref, torch.float32, f"rku{order}")
    got = PI.StructuredFunctionalAdapter(PT.UniPC(order=2)).sample_model(x0.to(dev), model_dev, PM.VelocityModel(), sched_p, 6)
    ref = OA.adapter_loop(OA.make("unipc", 2), x0, model_cpu, "v", sched_o, 6)
    assert_close(got, ref, torch.float32, "adapter unipc")


# ---- full-size properties (BASELINE shapes; the oracle only sees slices) -------------------------------
def test_full_size_properties(dev):
    B, C, H, W = 256, 4, 128, 128
    steps = 20
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))
    w.set_timesteps(steps)
    gd = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(B, C, H, W, device=dev, generator=gd).bfloat16()
    outs = [torch.randn(B, C, H, W, device=dev, generator=gd).bfloat16() for _ in range(3)]
    gens = [torch.Generator().manual_seed(42 + i) for i in range(B)]

    def run(xin, os_, gens_, lo=0, hi=B):
        ww = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))
        ww.set_timesteps(steps)
        cur, res = xin[lo:hi], []
        for i, o_ in enumerate(os_):
            cur = ww.step(o_[lo:hi], ww.timesteps[i], cur, generator=gens_[lo:hi], return_dict=False)[0]
            res.append(cur)
        return res

    full = run(x, outs, gens)
    again = run(x, outs, gens)
    for a, b in zip(full, again):
        assert torch.equal(a, b)  # deterministic (counter-based RNG, no atomics)
    # shard invariance: the halves of the batch, run separately, reproduce the full run bit for bit
    lo_half, hi_half = run(x, outs, gens, 0, B // 2), run(x, outs, gens, B // 2, B)
    for f, a, b in zip(full, lo_half, hi_half):
        assert torch.equal(f[: B // 2], a) and torch.equal(f[B // 2 :], b)
    # oracle on a few samples of the full-size run
    o = OW.StepDriver(OA.make("dpm", 2, eta=1), OS.karras(OS.scaled(), steps=steps), "eps")
    o.set_timesteps(steps)
    idx = [0, 1, 128, 255]
    xc = x[idx].cpu()
    n = C * H * W
    for i in range(3):
        noise = torch.from_numpy(np.stack([ON.philox_normal(42 + j, i * 256, n) for j in idx])).reshape(len(idx), C, H, W)
        ref = o.step(outs[i][idx].cpu(), o.timesteps[i], xc, noise=noise)[0]
        assert_close(full[i][idx], ref, torch.bfloat16, f"full-size step {i}")
        xc = full[i][idx].cpu()  # teacher-force: both sides see the device trajectory
    # linearity of the ODE step: step(a*x, a*out) == a*step(x, out) for a power of two (exact in bf16)
    e = PD.SkrampleWrapperScheduler(PT.DPM(order=1), PS.Scaled())
    e.set_timesteps(steps)
    y1 = e.step(outs[0], e.timesteps[0], x, return_dict=False)[0]
    e.set_timesteps(steps)
    y2 = e.step(outs[0] * 4, e.timesteps[0], x * 4, return_dict=False)[0]
    assert torch.equal(y2, y1 * 4)


FULL_SIZE = {
    # name: (wrapper factory, oracle factory, shape per GPU, calls)
    "cfg2_dpm2_sde_karras": (  # BASELINE config 2 as written: B = 64 on one GPU
        lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled())),
        lambda n, compute=torch.float32: OW.StepDriver(OA.make("dpm", 2, eta=1), OS.karras(OS.scaled(), steps=n), "eps", compute=compute),
        (64, 4, 128, 128),
        6,
    ),
    "headline_dpm2_sde_karras_b256": (  # the north-star shape of the same config
        lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled())),
        lambda n, compute=torch.float32: OW.StepDriver(OA.make("dpm", 2, eta=1), OS.karras(OS.scaled(), steps=n), "eps", compute=compute),
        (256, 4, 128, 128),
        5,
    ),
    "cfg3_unipc3_sde_flow": (
        lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Linear(), PM.FlowModel()),
        lambda n, compute=torch.float32: OW.StepDriver(OA.make("unipc", 3, eta=1), OS.linear(), "flow", compute=compute),
        (256, 16, 128, 128),
        5,
    ),
    "cfg4_adams4_v_zsnr": (
        lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.ZSNR(), PM.VelocityModel()),
        lambda n, compute=torch.float32: OW.StepDriver(OA.make("adams", 4), OS.zsnr(), "v", compute=compute),
        (256, 4, 128, 128),
        6,
    ),
    "cfg5_rkultra6_sde": (
        lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=6, stochasticity=1),
        lambda n, compute=torch.float32: OW.RKDriver(OK.pick_tableau(6), OS.scaled(), "eps", "data", 1.0, compute=compute),
        (64, 4, 256, 256),
        12,
    ),
}


@pytest.mark.parametrize("name", sorted(FULL_SIZE))
def test_full_size_baseline_configs(name, dev):
    """BASELINE configs 3-5 at their full per-GPU size: determinism, bitwise shard invariance (two half batches
    reproduce the whole), the oracle on a few samples of the full-size run (teacher-forced), and the oracle in float64 on the device
    over the whole batch (teacher-forced with the same inputs; its noise is PN.Random's, the Philox stream d * 256 the step kernels
    draw in-kernel, spot-checked against the specification on the three samples)."""
    mk_w, mk_o, shape, calls = FULL_SIZE[name]
    B, steps = shape[0], 20
    gd = torch.Generator(device=dev).manual_seed(4321)
    x = torch.randn(shape, device=dev, generator=gd).bfloat16()
    outs = [torch.randn(shape, device=dev, generator=gd).bfloat16() for _ in range(3)]
    seeds = [42 + i for i in range(B)]

    def run(lo, hi):
        w = mk_w()
        w.set_timesteps(steps)
        cur, ins, res = x[lo:hi], [], []
        for i in range(calls):
            o_ = (outs[i % 3][lo:hi] * 0.25 + cur * 0.5).bfloat16()  # a "network" that depends on the trajectory
            ins.append((cur, o_))
            cur = w.step(o_, w.timesteps[i], cur, generator=seeds[lo:hi], return_dict=False)[0]
            res.append(cur)
        return ins, res, w

    ins, full, w = run(0, B)
    _, again, _ = run(0, B)
    _, lo_half, _ = run(0, B // 2)
    _, hi_half, _ = run(B // 2, B)
    for f, a, l, h in zip(full, again, lo_half, hi_half):
        assert torch.equal(f, a) and torch.equal(f[: B // 2], l) and torch.equal(f[B // 2 :], h)
        assert torch.isfinite(f.float()).all()

    idx = [0, B // 2, B - 1]
    o = mk_o(steps)
    o.set_timesteps(steps)
    np.testing.assert_allclose(w.timesteps.numpy()[:calls], o.timesteps.numpy()[:calls], rtol=0, atol=1e-9)
    n = int(np.prod(shape[1:]))
    draws = iter(range(10**6))

    drawn3 = []

    def philox_noise(_step=None):
        d = next(draws)
        drawn3.append(torch.from_numpy(np.stack([ON.philox_normal(seeds[j], d * 256, n) for j in idx])).reshape(len(idx), *shape[1:]))
        return drawn3[-1]

    o64 = mk_o(steps, compute=torch.float64)
    o64.set_timesteps(steps)
    white = PN.BatchTensorNoise.from_batch_inputs(PN.Random, shape[1:], seeds, dtype=torch.float32)
    drawn = []

    def philox_noise_all(_step=None):
        "the whole batch's draw d (PN.Random: stream d * 256), its three samples checked against the specification's"
        got = white.generate(None)
        assert (got[idx].cpu().double() - drawn3[len(drawn)].double()).abs().max().item() < 4e-6, len(drawn)
        drawn.append(1)
        return got

    for i in range(calls):
        xin, oin = ins[i][0][idx].cpu(), ins[i][1][idx].cpu()
        if isinstance(o, OW.RKDriver):
            ref = o.step(oin, o.timesteps[i], xin, noise_fn=philox_noise)
            ref_all = o64.step(ins[i][1], o64.timesteps[i], ins[i][0], noise_fn=philox_noise_all)
        else:
            ref = o.step(oin, o.timesteps[i], xin, noise=philox_noise() if OA.require_noise(o.cfg) else None)[0]
            ref_all = o64.step(ins[i][1], o64.timesteps[i], ins[i][0], noise=philox_noise_all() if OA.require_noise(o64.cfg) else None)[0]
        assert_close(full[i][idx], ref, torch.bfloat16, f"{name} call {i}", flips=0.10)
        assert ref_all.dtype == torch.bfloat16 and ref_all.device == full[i].device
        assert_close(full[i], ref_all, torch.bfloat16, f"{name} call {i}, whole batch vs float64", flips=0.10)
        del ref_all
    assert len(drawn) == len(drawn3)
    del o64, ins, full, again, lo_half, hi_half
    torch.cuda.empty_cache()


def test_step_programs_replay_bitwise(dev):
    "second pass through a wrapper replays cached step programs: results identical to the first (algebra) pass"
    from skrample_amd.pytorch import noise as PN

    shape, steps = (3, 4, 32, 32), 8
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    outs = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(steps)]
    wrappers = [
        PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled())),
        PD.SkrampleWrapperScheduler(PT.DPM(order=3), PS.Scaled()),
        PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Linear(), PM.FlowModel()),
        PD.SkrampleWrapperScheduler(PT.UniPC(order=2, predictor=PT.Adams(order=3)), PS.Scaled(), PM.VelocityModel()),
        PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.ZSNR(), PM.VelocityModel()),
        PD.SkrampleWrapperScheduler(PT.Euler(stochasticity=1), PS.Scaled(), invert_prediction=True),
        PD.SkrampleWrapperScheduler(PT.SPC(), PS.Scaled()),
        PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Scaled(), noise_type=PN.Offset, noise_props=PN.OffsetProps()),
    ]
    # samplers whose step is not a fixed chain of step launches (SPC's signed-power blend) must opt out of programs
    unprogrammed = [
        PD.SkrampleWrapperScheduler(PT.SPC(power=2), PS.Scaled()),
        PD.SkrampleWrapperScheduler(PT.SPC(power=0.5, predictor=PT.DPM(order=2, stochasticity=0.5), corrector=PT.Adams(order=2)), PS.Linear(), PM.FlowModel()),
    ]
    for w in wrappers + unprogrammed:
        passes = []
        for rep in range(3):
            w.set_timesteps(steps)
            x, traj = x0, []
            for i, t in enumerate(w.timesteps):
                prev, pred = w.step(outs[i], t, x, generator=[5, 6, 7], return_dict=False)
                traj.append((prev, torch.as_tensor(pred.materialize() if isinstance(pred, lazy.LazyTensor) else pred)))
                x = prev
            passes.append(traj)
        cached = [k for k, v in w._programs.items() if v is not False]
        if w in unprogrammed:
            assert len(cached) <= 1, (type(w.sampler).__name__, len(cached))  # only the history-free first step is a plain launch
        else:
            assert len(cached) >= steps - 1, (type(w.sampler).__name__, len(cached))  # every step got a program
        for a, b, c in zip(*passes):
            assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], b[1]) and torch.equal(a[1], c[1]), type(w.sampler).__name__


def test_sampler_generics_device(dev):
    "reference test_sampler_generics: a python float and a (device, float64) tensor give the same step result"
    import random

    rnd = random.Random(0)
    for name, (_, mk_p) in SAMPLERS.items():
        sampler = mk_p()
        for schedule in (PS.Scaled(), PS.FlowShift(PS.Linear())):
            i, o, n = rnd.random(), rnd.random(), rnd.random()
            step = PT.Step.from_int(4, 10)
            prev_f = [PT.SKSamples(rnd.random(), rnd.random(), PT.Step((a := rnd.random()), a * 2), rnd.random(), rnd.random()) for _ in range(9)]
            f64 = lambda v: torch.tensor([v] * 8, dtype=torch.float64, device=dev)  # noqa: E731
            prev_t = [PT.SKSamples(f64(p.sample), f64(p.prediction), p.step, f64(p.noise), f64(p.final)) for p in prev_f]
            scalar = sampler.sample(i, o, step, PM.DataModel(), schedule, n, previous=prev_f).final
            tensor = sampler.sample(f64(i), f64(o), step, PM.DataModel(), schedule, f64(n), previous=prev_t).final
            assert tensor.dtype == torch.float64 and abs(tensor[0].item() - scalar) < 1e-12 * max(1.0, abs(scalar)), (name, tensor[0].item(), scalar)


@pytest.mark.parametrize("wrapper", [PD.RKUltraWrapperScheduler, PD.DynasauRKWrapperScheduler])
def test_runge_kutta_wrapper_equals_functional(wrapper, dev):
    """reference test_runge_kutta_diffusers (tests/self_sampling.py:417-500): the inside-out wrapper reproduces the
    functional sampler model call by model call -- points to 1e-15, samples to 1e-8 -- over models, derivative
    transforms, orders and stochasticities.  Functional side runs on python floats, wrapper side on float64
    device tensors (compute_scale=float64), noise injected."""
    import itertools
    import math
    import random

    from skrample_amd.common import Point

    rnd = random.Random(7)
    combos = itertools.product(
        [PM.DataModel, PM.VelocityModel, PM.FlowModel],
        [None, PM.DataModel, PM.VelocityModel, PM.FlowModel, PM.ScaleX],
        [PS.Sinner(PS.Linear()), PS.Scaled()],
        [0, 2, 3, 4, 6] if wrapper is PD.RKUltraWrapperScheduler else [2, 3, 4],
        [0, 0.5, -1.5],
    )
    for model, transform, schedule, order, eta in combos:
        if rnd.random() > 0.2:  # a seeded fifth of the full product keeps this under a few seconds
            continue
        w = wrapper(schedule, sampler_order=order, stochasticity=eta, model=model(), derivative_transform=transform() if transform else None, compute_scale=torch.float64)
        steps = rnd.randint(3, 9)
        fake = lambda x, t, s, a: x + math.sin(x) * s  # noqa: E731
        seen_ref, pts_ref = [], []

        def model_ref(x, t, s, a):
            seen_ref.append(x)
            pts_ref.append(Point(t, s, a))
            return fake(x, t, s, a)

        noises = [rnd.gauss(0, 1) for _ in range(steps)]
        it = iter(noises)
        x0 = 1 / (rnd.random() + 1e-4) * (rnd.randint(0, 1) * 2 - 1)
        want = w.functional_sample_model(x0, model_ref, steps, rng=lambda _: next(it))

        w.set_timesteps(steps)
        w._noise_generator = Injected([torch.full((1, 8), v, dtype=torch.float64) for v in noises], dev)
        x = x0
        for n, (t, sg) in enumerate(zip(w.timesteps, w.sigmas)):
            s_n, a_n = (v.item() for v in w.schedule.space.normalize(sg.item()))
            np.testing.assert_allclose((t.item(), s_n, a_n), pts_ref[n], rtol=0, atol=1e-12)
            assert abs(seen_ref[n] - x) < 1e-8 * max(1, abs(x)), (model.__name__, transform, order, eta, n)
            out = fake(x, t.item(), s_n, a_n)
            res = w.step(torch.full((1, 8), out, dtype=torch.float64, device=dev), t, torch.full((1, 8), x, dtype=torch.float64, device=dev), return_dict=False)[0]
            assert res.dtype == torch.float64
            x = res[0, 0].item()
        assert abs(want - x) < 1e-8 * max(1, abs(want)), (model.__name__, transform, order, eta)


def test_rk_stage_programs_replay_bitwise(dev):
    "the Runge-Kutta wrappers replay cached stage launches on later passes: identical results"
    from skrample_amd.pytorch import noise as PN

    shape, steps = (2, 4, 32, 32), 4
    g = torch.Generator().manual_seed(12)
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    pool = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(steps * 6)]
    wrappers = [
        PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=6, stochasticity=1),
        PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=4, stochasticity=0.5, model=PM.VelocityModel()),
        PD.RKUltraWrapperScheduler(PS.Linear(), sampler_order=2, model=PM.FlowModel()),
        PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=5, derivative_transform=None),
        PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=3, stochasticity=1, noise_type=PN.Pyramid, noise_props=PN.PyramidProps()),
        PD.DynasauRKWrapperScheduler(PS.Scaled(), sampler_order=3, stochasticity=1),
    ]
    for w in wrappers:
        passes = []
        for rep in range(3):
            w.set_timesteps(steps)
            x, traj = x0, []
            for i, t in enumerate(w.timesteps):
                x, pred = w.step(pool[i], t, x, generator=[5, 6], return_dict=False)
                traj.append((x, torch.as_tensor(pred.materialize() if isinstance(pred, lazy.LazyTensor) else pred)))
            passes.append(traj)
        cached = [k for k, v in w._rk_programs.items() if v]
        assert len(cached) >= len(passes[0]) - w.order, (type(w).__name__, w.sampler_order, len(cached), len(passes[0]))
        for a, b, c in zip(*passes):
            assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and torch.equal(a[1], b[1]) and torch.equal(a[1], c[1]), (type(w).__name__, w.sampler_order)


def test_alias_history_off_survives_buffer_reuse(dev):
    "with alias_history=False the caller may overwrite sample / model_output in place between steps"
    shape, steps = (2, 4, 16, 16), 6
    g = torch.Generator().manual_seed(13)
    x0 = torch.randn(shape, generator=g).to(dev)
    outs = [torch.randn(shape, generator=g).to(dev) for _ in range(steps)]
    for mk in (lambda **k: PD.SkrampleWrapperScheduler(PT.DPM(order=3), PS.Scaled(), **k), lambda **k: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=4, **k)):
        ref_w, w = mk(), mk(alias_history=False)
        ref_w.set_timesteps(steps)
        w.set_timesteps(steps)
        x_ref = x0.clone()
        static_x, static_out = x0.clone(), torch.empty_like(x0)  # one pair of buffers reused for every call
        for i, t in enumerate(w.timesteps):
            x_ref = ref_w.step(outs[i % steps].clone(), t, x_ref, return_dict=False)[0]
            static_out.copy_(outs[i % steps])
            res = w.step(static_out, t, static_x, return_dict=False)[0]
            static_x.copy_(res)
            assert torch.equal(res, x_ref), i


def test_device_timesteps_are_located_not_assumed(dev):
    """device-resident timesteps used to be trusted to arrive in schedule order.  An element of the `timesteps`
    tensor the scheduler handed out is now recognised by its storage offset (no .item() sync), so a pipeline that slices,
    repeats or skips steps gets the coefficients of the step it names; a foreign device scalar is read back once, as in the
    reference (diffusers.py:565-567)."""
    shape, steps = (2, 4, 16, 16), 8
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(shape, generator=g).to(dev)
    outs = [torch.randn(shape, generator=g).to(dev) for _ in range(steps)]
    mk = lambda: PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled())  # noqa: E731

    def run(kind):
        w = mk()
        w.set_timesteps(steps, device=dev)
        ts_dev, ts_host = w.timesteps, w.timesteps.tolist()
        x = x0
        for i in (0, 1, 2, 5, 6):  # a pipeline that skips steps 3-4 without set_begin_index
            t = {"host": ts_host[i], "view": ts_dev[i], "foreign": torch.tensor(ts_host[i], dtype=ts_dev.dtype, device=dev)}[kind]
            x = w.step(outs[i], t, x, return_dict=False)[0]
        return x

    ref = run("host")
    assert torch.equal(run("view"), ref) and torch.equal(run("foreign"), ref)
    w = mk()
    w.set_timesteps(steps, device=dev)
    with pytest.raises(ValueError):
        w.step(outs[0], torch.tensor(123.456, dtype=torch.float64, device=dev), x0)  # not a timestep of this schedule
    rk = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=2)
    rk.set_timesteps(4, device=dev)
    ts = rk.timesteps
    rk.step(outs[0], ts[0], x0)
    with pytest.raises(AssertionError):
        rk.step(outs[1], ts[2], x0)  # out of order: the reference asserts on the value, here the position is checked


def test_stage_replay_fallback_keeps_the_noise_stream(dev):
    """a stage replay that bailed out AFTER drawing the step noise left the generator one draw ahead, so the normal
    path drew stream (n+1)*256.  Operands are now validated before the draw (and a draw already made is handed over): a run whose
    final stages cannot be replayed (non-contiguous network output) must equal the run that replays everything, bit for bit."""
    shape, steps, seeds = (2, 4, 32, 32), 3, [5, 6]
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    n_calls = 3 * steps * 4
    outs = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(n_calls)]
    wide = [torch.randn(shape[0], shape[1], shape[2], 2 * shape[3], generator=g).bfloat16().to(dev) for _ in range(n_calls)]
    for o, wd in zip(outs, wide):
        wd[..., ::2] = o  # the same values behind a strided (non-contiguous) view

    def run(strided_final: bool):
        w = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=4, stochasticity=1.0)
        result = None
        for rep in range(2):  # second pass: every stage has a recorded program
            w.set_timesteps(steps)
            x = x0
            ts = w.timesteps.tolist()
            for i, t in enumerate(ts):
                final_stage = (i + 1) % w.order == 0
                out = wide[i][..., ::2] if (strided_final and final_stage and rep == 1) else outs[i]
                x = w.step(out, t, x, generator=seeds, return_dict=False)[0]
            result = x
        return result, w._noise_generator._draws

    ref, draws_ref = run(False)
    got, draws_got = run(True)
    assert draws_got == draws_ref
    assert torch.equal(got, ref)


def test_aliased_history_is_guarded(dev):
    """alias_history=True keeps the caller's tensors as history operands (the reference deep-copies, structured.py:113-125):
    a caller that reuses its buffers must get an error, never a silently wrong step; alias_history=False snapshots and must
    then reproduce the result of a run on fresh tensors bit for bit; the default ("auto") finds out which caller it has and
    never raises for the two static-buffer patterns (test_alias_auto_* below)."""
    shape, steps = (2, 4, 16, 16), 6
    g = torch.Generator().manual_seed(77)
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    outs = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(steps)]
    mk = lambda **kw: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), **kw)  # noqa: E731

    def run(w, reuse):
        w.set_timesteps(steps)
        x, buf = x0, torch.empty_like(outs[0])
        for i, t in enumerate(w.timesteps.tolist()):
            out = outs[i]
            if reuse == "copy_":  # one network-output buffer, rewritten in place every step (version bump)
                buf.copy_(out)
                out = buf
            elif reuse == "static":  # a graphed network: same storage, new tensor object, no version bump
                buf.view(torch.int16).untyped_storage().copy_(out.view(torch.int16).untyped_storage())
                out = buf.view(shape)
            x = w.step(out, t, x, generator=[1, 2], return_dict=False)[0]
        return x

    fresh = run(mk(alias_history=True), None)
    assert torch.equal(run(mk(), None), fresh)  # default ("auto") on fresh tensors: same bits
    for reuse in ("copy_", "static"):
        with pytest.raises(_hip.SkrampleHipError, match="alias_history=False"):
            run(mk(alias_history=True), reuse)
        assert torch.equal(run(mk(alias_history=False), reuse), fresh)
        w = mk()
        assert torch.equal(run(w, reuse), fresh)  # the default no longer throws where the reference works
        assert w._alias_auto == "snapshot"
    w = mk()
    run(w, None)
    assert w._alias_auto == "alias"  # fresh tensors every step: history entries are the caller's own tensors (0 bytes written)
    # in-place edit of the latents between steps
    w = mk(alias_history=True)
    w.set_timesteps(steps)
    ts = w.timesteps.tolist()
    x = w.step(outs[0], ts[0], x0.clone(), generator=[1, 2], return_dict=False)[0]
    w._alias_stamps[0][0].mul_(1.0)  # the first step's sample, touched in place by the caller
    with pytest.raises(_hip.SkrampleHipError, match="modified in place"):
        w.step(outs[1], ts[1], x, generator=[1, 2], return_dict=False)
    # samplers without history hold nothing
    w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled())
    w.set_timesteps(3)
    buf, x = outs[0].clone(), x0
    for t in w.timesteps.tolist():
        x = w.step(buf, t, x, return_dict=False)[0]
    # Runge-Kutta stages: the step's base sample is held until the last stage
    rk = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=4, alias_history=True)
    rk.set_timesteps(3)
    ts = rk.timesteps.tolist()
    base = x0.clone()
    nxt = rk.step(outs[0], ts[0], base, return_dict=False)[0]
    base.add_(1.0)
    with pytest.raises(_hip.SkrampleHipError, match="modified in place"):
        rk.step(outs[1], ts[1], nxt, return_dict=False)


def test_alias_auto_static_output_network_loops(dev):
    """The default wrappers run a loop whose network writes every output into ONE static buffer (a HIP-graphed network, an
    in-place copy_) without raising, for multistep and Runge-Kutta samplers alike, and reproduce the fresh-tensor run bit for
    bit; a second run of the same wrapper (set_timesteps) decides afresh."""
    shape, steps = (2, 4, 16, 16), 5
    g = torch.Generator().manual_seed(78)
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    outs = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(steps * 6)]
    makers = [
        lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Linear(), PM.FlowModel()),
        lambda: PD.SkrampleWrapperScheduler(PT.Adams(order=4), PS.ZSNR(), PM.VelocityModel()),
        lambda: PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=6, stochasticity=1),
        lambda: PD.DynasauRKWrapperScheduler(PS.Scaled(), sampler_order=3),
    ]
    for mk in makers:
        def run(w, static, latents_static=False):
            w.set_timesteps(steps)
            x, buf, lat = x0, torch.empty_like(outs[0]), x0.clone()
            for i, t in enumerate(w.timesteps.tolist()):
                out = outs[i]
                if static:
                    buf.copy_(out)
                    out = buf
                if latents_static:  # the pipeline keeps ONE latents buffer too
                    lat.copy_(x)
                    x = lat
                x = w.step(out, t, x, generator=[1, 2], return_dict=False)[0]
            return x.clone()

        fresh = run(mk(), False)
        w = mk()
        assert torch.equal(run(w, True), fresh) and w._alias_auto == "snapshot"
        assert torch.equal(run(w, False), fresh) and w._alias_auto == "alias"  # next run, other caller behaviour
        assert torch.equal(run(mk(), False, latents_static=True), fresh)


def test_whole_loop_graph_capture(dev):
    "an N-step loop (toy network + fused DPM-2 SDE steps) recorded into one HIP graph replays bit-identically"
    from skrample_amd.graphs import capture_sampling_loop

    shape, steps, seeds = (4, 4, 32, 32), 8, [3, 4, 5, 6]
    g = torch.Generator().manual_seed(14)
    weight = (torch.randn(32, 32, generator=g) * 0.05).to(dev).bfloat16()
    net = lambda x, t: (x @ weight) + x * (t / 1000)  # noqa: E731
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)

    def eager(x, sd):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))
        w.set_timesteps(steps)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=sd, return_dict=False)[0]
        return x

    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))
    loop = capture_sampling_loop(w, net, x0, steps, seeds=seeds)
    assert torch.equal(loop(x0), eager(x0, seeds))
    x1 = torch.randn(shape, generator=g).bfloat16().to(dev)
    assert torch.equal(loop(x1), eager(x1, seeds))  # new latents, same graph
    assert torch.equal(loop(x1, seeds=[9, 8, 7, 6]), eager(x1, [9, 8, 7, 6]))  # new seeds are read from device memory


def _oracle_loop(cfg, sched_name, pred, net, x0, steps, seeds):
    "the same N-step loop on the oracle (CPU), fed the Philox normals the kernels draw (stream = 256 * step)"
    o = OW.StepDriver(cfg, oracle_schedule(sched_name, steps), pred)
    o.set_timesteps(steps)
    x, n = x0.clone(), x0[0].numel()
    for i, t in enumerate(o.timesteps.tolist()):
        noise = torch.from_numpy(np.stack([ON.philox_normal(sd, i * 256, n) for sd in seeds])).reshape(x0.shape)
        x = o.step(net(x, t), t, x, noise=noise)[0]
    return x


@pytest.mark.parametrize("indexed", [False, True])
def test_whole_loop_graph_capture_vs_oracle(indexed, dev):
    """the captured loop (frozen kernel arguments, or device-resident step scalars) against the ORACLE's trajectory of the same
    loop -- fp32 latents and an elementwise network, so both sides carry only fp32 rounding -- and bitwise against eager"""
    from skrample_amd.graphs import capture_sampling_loop

    shape, steps, seeds = (4, 4, 32, 32), 9, [3, 4, 5, 6]
    g = torch.Generator().manual_seed(21)
    net = lambda x, t: x * 0.75 - (t / 2000) * x.abs()  # noqa: E731
    x0 = torch.randn(shape, generator=g)
    mk = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))  # noqa: E731
    loop = capture_sampling_loop(mk(), net, x0.to(dev), steps, seeds=seeds, indexed=indexed)
    got = loop(x0.to(dev))
    w = mk()
    w.set_timesteps(steps)
    x = x0.to(dev)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=seeds, return_dict=False)[0]
    assert torch.equal(got, x)
    ref = _oracle_loop(OA.make("dpm", 2, eta=1), "karras_scaled", "eps", net, x0, steps, seeds)
    assert rel_err(got, ref) < 5e-5, rel_err(got, ref)  # 9 chained steps of <= 1e-5 each (Philox normals within 2e-6)


def test_captured_loops_serve_any_run_length(dev):
    """the reference's loop takes `steps` per call (interface.py:34-59): CapturedLoops records one graph per run length on first use,
    replays it afterwards, keeps the most recently used lengths -- every length equals the eager run of that length bit for bit, with the
    seeds given at the call"""
    from skrample_amd.graphs import CapturedLoops

    shape = (3, 4, 16, 16)
    g = torch.Generator().manual_seed(77)
    net = lambda x, t: x * 0.75 - (t / 2000) * x.abs()  # noqa: E731
    x0 = torch.randn(shape, generator=g).to(dev)
    mk = lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Karras(PS.Scaled()))  # noqa: E731

    def eager(steps, seeds, x):
        w = mk()
        w.set_timesteps(steps)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=list(seeds), return_dict=False)[0]
        return x

    loops = CapturedLoops(mk, net, x0, seeds=[1, 2, 3], keep=2)
    for steps, seeds in ((5, [1, 2, 3]), (9, [4, 5, 6]), (5, [7, 8, 9]), (2, [1, 2, 3]), (9, [1, 2, 3])):
        x = torch.randn(shape, generator=g).to(dev)
        assert torch.equal(loops(x, steps, seeds=seeds), eager(steps, seeds, x)), steps
    assert loops.captures == 4 and loops.resident == (2, 9)  # 5, 9 recorded; 5 replayed; 2 recorded (9, the least recently used, dropped); 9 recorded again (5 dropped)
    with pytest.raises(ValueError):
        loops(x0, 0)


@pytest.mark.parametrize("kind", ["dpm2_sde", "unipc3_sde", "adams4", "rk4_sde", "adams7", "unipc5_sde"])
def test_indexed_graph_serves_other_schedules(kind, dev):
    """skr_step_launch_indexed: one captured loop, step scalars resident on the device.  Re-targeting it to other schedules of
    the same length (other sigmas, other base schedule, other stochasticity) only rewrites rows -- no re-capture -- and must
    reproduce the eager run of that scheduler bit for bit; several schedules stay resident and are picked by the device index."""
    from skrample_amd.graphs import capture_sampling_loop

    shape, steps, seeds = (4, 4, 32, 32), (10 if kind in ("adams7", "unipc5_sde") else 6), [11, 12, 13, 14]
    g = torch.Generator().manual_seed(31)
    # (the toy network ignores t: a host float t would be frozen into the graph; real pipelines feed the device-resident
    #  `scheduler.timesteps`, which is data like the rows)
    net = lambda x, t: x * 0.5 + 0.3 * x.abs()  # noqa: E731
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    makers = {
        "dpm2_sde": lambda sch, eta=1.0: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=eta), sch),
        "unipc3_sde": lambda sch, eta=1.0: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=eta), sch),
        "adams4": lambda sch, eta=0.0: PD.SkrampleWrapperScheduler(PT.Adams(order=4), sch),
        "rk4_sde": lambda sch, eta=1.0: PD.RKUltraWrapperScheduler(sch, sampler_order=4, stochasticity=eta),
        # round 3: the table forms of the 9-16-operand compile-time kernels (a device-resident row holds 16 operands)
        "adams7": lambda sch, eta=0.0: PD.SkrampleWrapperScheduler(PT.Adams(order=7), sch),
        "unipc5_sde": lambda sch, eta=1.0: PD.SkrampleWrapperScheduler(PT.UniPC(order=5, stochasticity=eta), sch),
    }
    mk = makers[kind]
    variants = [PS.Karras(PS.Scaled()), PS.Scaled(), PS.Karras(PS.Scaled(), rho=3.0), PS.Exponential(PS.Scaled())]

    def eager(w, x):
        w.set_timesteps(steps)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=seeds, return_dict=False)[0]
        return x

    loop = capture_sampling_loop(mk(variants[0]), net, x0, steps, seeds=seeds, indexed=True, slots=4)
    assert torch.equal(loop(x0), eager(mk(variants[0]), x0))
    for slot, sch in enumerate(variants[1:], start=1):
        loop.retarget(mk(sch), slot=slot)
    outs = [loop(x0, slot=k) for k in range(4)]
    for k, sch in enumerate(variants):
        assert torch.equal(outs[k], eager(mk(sch), x0)), (kind, k)
    assert not torch.equal(outs[0], outs[1])
    if kind not in ("adams4", "adams7"):  # another stochasticity is just other zeta / gamma values in the rows
        loop.retarget(mk(variants[1], 0.5), slot=0)
        assert torch.equal(loop(x0, slot=0), eager(mk(variants[1], 0.5), x0))
    x1 = torch.randn(shape, generator=g).bfloat16().to(dev)
    assert torch.equal(loop(x1, slot=2), eager(mk(variants[2]), x1))  # new latents, resident schedule 2
    with pytest.raises(_hip.SkrampleHipError):  # a structurally different sampler cannot reuse the capture
        loop.retarget(PD.SkrampleWrapperScheduler(PT.Euler(), PS.Scaled()), slot=3)


def test_indexed_launch_through_the_c_abi(dev):
    "skr_step_launch_indexed directly: rows on the device, the index picks the row at run time; unsupported shapes are refused"
    lib = _hip.load()
    batch, sample = 2, 4096
    n = batch * sample
    g = torch.Generator().manual_seed(5)
    ins = [torch.randn(n, generator=g).bfloat16().to(dev) for _ in range(3)]
    seeds = torch.tensor([7, 8], dtype=torch.int64, device=dev)
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.out0_dtype, plan.out1_dtype = 3, 3, _hip.BF16, _hip.BF16, _hip.BF16, -1
    plan.noise_mode, plan.sample_numel = 1, sample
    rows = (_hip.StepRowC * 3)()
    for r, row in enumerate(rows):
        for k in range(3):
            row.coef0[k] = 0.25 * (k + 1) * (-1) ** r
        row.zeta0, row.stream0 = (0.5, 4 + r) if r < 2 else (0.0, 0)
    rows_dev = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    index = torch.zeros(1, dtype=torch.int32, device=dev)
    ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ins])
    stream = torch.cuda.current_stream(dev).cuda_stream
    for idx, off in ((0, 0), (1, 0), (0, 2), (1, 1)):
        index.fill_(idx)
        r = idx + off
        got = torch.empty(n, device=dev, dtype=torch.bfloat16)
        assert lib.skr_step_launch_indexed(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, rows_dev.data_ptr(), index.data_ptr(), off, stream) == 0
        ref_plan = _hip.StepPlanC()
        ctypes.memmove(ctypes.byref(ref_plan), ctypes.byref(plan), ctypes.sizeof(plan))
        for k in range(3):
            ref_plan.coef0[k] = rows[r].coef0[k]
        ref_plan.zeta0, ref_plan.stream0 = rows[r].zeta0, rows[r].stream0
        ref = torch.empty_like(got)
        _hip.launch_step(ref_plan, ins, ref, None, seeds, n, dev)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), (idx, off)
    ragged = n - 8  # not made of whole chunks: the one-trip kernels do not cover it
    assert lib.skr_step_launch_indexed(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), ragged - ragged % sample, rows_dev.data_ptr(), index.data_ptr(), 0, stream) in (0, 7)
    plan.sample_numel = 8 * 33
    assert lib.skr_step_launch_indexed(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), 8 * 33 * 2, rows_dev.data_ptr(), index.data_ptr(), 0, stream) == 7  # SKR_ERR_UNSUPPORTED
    assert lib.skr_step_launch_indexed(ctypes.byref(plan), ptrs, got.data_ptr(), None, seeds.data_ptr(), n, None, None, 0, stream) == 1  # SKR_ERR_NULL


@pytest.mark.parametrize("noise", ["Offset", "Pyramid", "Colored", "Brownian"])
def test_whole_loop_graph_capture_structured_noise(noise, dev):
    "every generator is a fixed chain of launches on the caller's stream (no host read-back), so loops that use them capture too"
    from skrample_amd.graphs import capture_sampling_loop
    from skrample_amd.pytorch import noise as PN

    kind = getattr(PN, noise)
    shape, steps, seeds = (3, 4, 32, 32), 5, [3, 4, 5]
    g = torch.Generator().manual_seed(16)
    net = lambda x, t: x * (0.5 + t / 2000)  # noqa: E731
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)
    mk = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()), noise_type=kind)  # noqa: E731

    def eager(x, sd):
        w = mk()
        w.set_timesteps(steps)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=sd, return_dict=False)[0]
        return x

    loop = capture_sampling_loop(mk(), net, x0, steps, seeds=seeds)
    assert torch.equal(loop(x0), eager(x0, seeds))
    assert torch.equal(loop(x0, seeds=[7, 8, 9]), eager(x0, [7, 8, 9]))
    assert not torch.equal(loop(x0, seeds=[7, 8, 9]), loop(x0, seeds=seeds))


@pytest.mark.parametrize(("wrapper_type", "kw"), [(PD.RKUltraWrapperScheduler, {"sampler_order": 6, "stochasticity": 1.0}), (PD.DynasauRKWrapperScheduler, {"sampler_order": 3})])
def test_whole_loop_graph_capture_runge_kutta(wrapper_type, kw, dev):
    "the RK wrappers' stage loop (6 network calls per step for Cash-Karp) is capturable too and replays bit-identically"
    from skrample_amd.graphs import capture_sampling_loop

    shape, steps, seeds = (3, 4, 16, 32), 4, [3, 4, 5]
    g = torch.Generator().manual_seed(15)
    weight = (torch.randn(32, 32, generator=g) * 0.05).to(dev).bfloat16()
    net = lambda x, t: (x @ weight) + x * (t / 1000)  # noqa: E731
    x0 = torch.randn(shape, generator=g).bfloat16().to(dev)

    def eager(x, sd):
        w = wrapper_type(PS.Scaled(), **kw)
        w.set_timesteps(steps)
        for t in w.timesteps.tolist():
            x = w.step(net(x, t), t, x, generator=sd, return_dict=False)[0]
        return x

    w = wrapper_type(PS.Scaled(), **kw)
    loop = capture_sampling_loop(w, net, x0, steps, seeds=seeds)
    assert len(w.timesteps) >= steps * 2
    assert torch.equal(loop(x0), eager(x0, seeds))
    x1 = torch.randn(shape, generator=g).bfloat16().to(dev)
    assert torch.equal(loop(x1), eager(x1, seeds))
    if kw.get("stochasticity"):
        assert torch.equal(loop(x1, seeds=[9, 8, 7]), eager(x1, [9, 8, 7]))


@pytest.mark.parametrize("name", ["Stepanov10", "Feagin14"])
def test_many_stage_runge_kutta(name, dev):
    """15- and 35-stage tableaux through the RK wrapper: launches with up to 37 operands vs the oracle.
    These tableaux have large coefficients of alternating sign, so an fp32 evaluation (the reference's as much as
    ours) carries cancellation noise above 1e-5; the arithmetic is therefore checked strictly in float64
    (<= 1e-10) and in float32 against the float64 truth with the reference's own fp32 error as the yardstick."""
    from skrample_amd.sampling import tableaux as PTab

    tab = getattr(PTab.RKZ, name).tableau()
    stages = len(tab.stages)
    otab = (tuple((s.c, tuple(s.a)) for s in tab.stages), tuple(tab.weights))  # coefficients are pinned by tests/golden/tables.json
    g = torch.Generator().manual_seed(15)
    shape = (2, 4, 16, 16)
    noises = [torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(2)]
    x0 = torch.randn(shape, generator=g, dtype=torch.float64)
    outs = [torch.randn(shape, generator=g, dtype=torch.float64) * 0.1 for _ in range(2 * stages)]

    def run(dtype):
        w = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=stages, stochasticity=0.5, providers={stages: getattr(PTab.RKZ, name)}, compute_scale=dtype)
        o = OW.RKDriver(otab, OS.scaled(), "eps", "data", 0.5, compute=dtype)
        w.set_timesteps(2)
        o.set_timesteps(2)
        assert w.order == stages and torch.equal(w.timesteps, o.timesteps)
        w._noise_generator = Injected([n.to(dtype) for n in noises], dev)
        pending = [n.to(dtype) for n in noises]
        x, got_all, ref_all = x0.to(dtype), [], []
        for i, t in enumerate(w.timesteps):
            out = outs[i].to(dtype) + x * 0.5
            got_all.append(w.step(out.to(dev), t, x.to(dev), return_dict=False)[0].cpu())
            ref_all.append(o.step(out, t, x, noise_fn=lambda st: pending.pop(0)))
            x = ref_all[-1]
        return got_all, ref_all

    got64, ref64 = run(torch.float64)
    for i, (a, b) in enumerate(zip(got64, ref64)):
        assert rel_err(a, b) <= 1e-10, (name, i, rel_err(a, b))
    got32, ref32 = run(torch.float32)
    for i, (a, b, truth) in enumerate(zip(got32, ref32, ref64)):
        ours, theirs = rel_err(a, truth), rel_err(b, truth)
        assert ours <= max(REL_TOL_F32, 2 * theirs), (name, i, ours, theirs)


@pytest.mark.parametrize("seed", range(24))
def test_random_sweep_runge_kutta_vs_oracle(seed, dev):
    "seeded random draw over (RK order x schedule x predictor x eta x dtype x ragged shape) through RKUltraWrapperScheduler"
    import random

    rng = random.Random(500 + seed)
    order = rng.randint(1, 6)
    if rng.random() < 0.4:
        sname, mname = rng.choice(("linear", "flowshift_linear", "sinner_linear")), rng.choice(("flow", "data", "v"))
    else:
        sname, mname = rng.choice(("scaled", "hyper_scaled", "scaled_neg_b1")), rng.choice(("eps", "v", "data"))
    eta = rng.choice((0.0, 0.0, 0.5, 1.0))
    dtype = rng.choice((torch.float32, torch.float32, torch.bfloat16, torch.float16))
    shape = (rng.randint(1, 3), rng.randint(1, 4), rng.choice((8, 13, 16)), rng.choice((8, 10, 17)))
    steps = rng.randint(2, 5)
    g = torch.Generator().manual_seed(seed)
    w = PD.RKUltraWrapperScheduler(SCHEDULES[sname][1](), sampler_order=order, stochasticity=eta, model=MODELS[mname][1])
    o = OW.RKDriver(OK.pick_tableau(order), SCHEDULES[sname][0](), MODELS[mname][0], "data", eta)
    w.set_timesteps(steps)
    o.set_timesteps(steps)
    np.testing.assert_allclose(w.timesteps.numpy(), o.timesteps.numpy(), rtol=0, atol=1e-9)
    noises = [torch.randn(shape, generator=g) for _ in range(steps)]
    w._noise_generator = Injected(noises, dev)
    pending = list(noises)
    x = torch.randn(shape, generator=g).to(dtype)
    what = f"rk{order}/{sname}/{mname}/eta{eta}/{dtype}/{shape}/{steps}"
    for i, t in enumerate(w.timesteps):
        out = (torch.randn(shape, generator=g) * 0.2 + x.float() * 0.5).to(dtype)
        ref = o.step(out, t, x, noise_fn=lambda st: pending.pop(0))
        got = w.step(out.to(dev), t, x.to(dev), return_dict=False)[0]
        if not torch.isfinite(ref.float()).all():
            return
        # (a 6-stage combination sums up to 9 terms in a different order than the reference: a few more last-place
        #  flips than a multistep update, every one still within one unit in the last place)
        assert_close(got, ref, dtype, f"{what} call {i}", flips=0.10)
        x = ref


def test_step_tableau_inside_out_entry(dev):
    "the reference-named stage method of the RK wrappers (diffusers.py:746-796) used directly: Heun = two feeds per step"
    w = PD.RKUltraWrapperScheduler(PS.Scaled(), sampler_order=2, model=PM.DataModel(), providers={2: PD.tableaux.RKE2.Heun})
    w.set_timesteps(4)
    g = torch.Generator().manual_seed(2)
    x, d0, d1 = (torch.randn(2, 4, 8, 8, generator=g).to(dev) for _ in range(3))
    pts = [PS.Point(*row) for row in w.schedule_np]
    s0, s1 = w.schedule.ipoint(0.0), w.schedule.ipoint(0.25)
    mid = w.step_tableau_inside_out(x, d0, PM.DataModel(), s0, s1, s1, None)
    fin = w.step_tableau_inside_out(mid, d1, PM.DataModel(), s0, s1, s1, None)
    from skr_oracle import predictors as OP

    p0, p1 = OS.scaled().ipoint(0.0), OS.scaled().ipoint(0.25)
    ref_mid = OP.forward("data", x.cpu(), d0.cpu(), p0, p1)
    ref_fin = OP.forward("data", x.cpu(), 0.5 * d0.cpu() + 0.5 * d1.cpu(), p0, p1)
    assert_close(mid, ref_mid, torch.float32, "stage input")
    assert_close(fin, ref_fin, torch.float32, "step result")
    assert w._derivatives == [] and w._sample is None and len(pts) >= 4


def test_img2img_entry_points(dev):
    "scale_noise / add_noise / set_begin_index: the img2img path (reference diffusers.py:375-381,540-543)"
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Scaled())
    w.set_timesteps(10)
    g = torch.Generator().manual_seed(16)
    clean, noise = torch.randn(2, 4, 16, 16, generator=g), torch.randn(2, 4, 16, 16, generator=g)
    t = w.timesteps[4]
    p = w.schedule.schedule(10)[4]
    noisy = w.scale_noise(clean.to(dev), t, noise.to(dev))
    assert_close(noisy, clean * p.alpha + noise * p.sigma, torch.float32, "scale_noise")
    assert_close(w.add_noise(clean.to(dev), noise.to(dev), w.timesteps[4:5]), clean * p.alpha + noise * p.sigma, torch.float32, "add_noise")
    assert w.add_noise(clean.to(dev), noise.to(dev), w.timesteps[:0]).cpu().equal(clean)
    # start in the middle of the schedule with device-resident timesteps (no host sync): begin index drives the order
    w.set_timesteps(10, device=dev)
    w.set_begin_index(4)
    o = OW.StepDriver(OA.make("dpm", 2), OS.scaled(), "eps")
    o.set_timesteps(10)
    x = noisy.cpu()
    for i in range(4, 10):
        out = torch.randn(2, 4, 16, 16, generator=g)
        got = w.step(out.to(dev), w.timesteps[i], x.to(dev), return_dict=False)[0]
        ref = o.step(out, o.timesteps[i], x)[0]
        assert_close(got, ref, torch.float32, f"begin_index step {i}")
        x = ref
    assert w.config["begin_index"] == 4


def test_rkmoire_on_device(dev):
    "adaptive RK on device tensors: embedded pair from one launch, error norms by the reduction kernel, vs the oracle"
    from skrample_amd.sampling import functional as PF

    g = torch.Generator().manual_seed(17)
    wmat = torch.randn(16, 16, generator=g, dtype=torch.float64) * 0.05
    for dtype, tol in ((torch.float64, 1e-10), (torch.float32, REL_TOL_F32)):
        x0 = torch.randn(2, 4, 16, 16, generator=g, dtype=torch.float64).to(dtype)
        wc, wd = wmat.to(dtype), wmat.to(dtype).to(dev)
        for order, (sp, so), (pp, po) in ((2, SCHEDULES["scaled"], (PM.VelocityModel(), "v")), (4, SCHEDULES["linear"], (PM.FlowModel(), "flow")), (6, SCHEDULES["scaled"], (PM.DataModel(), "data"))):
            seen_o, seen_p = [], []
            ref = OK.rkmoire_loop(x0, lambda x, t, s, a: x @ wc + x * s, po, sp(), 24, order=order, callback=lambda x, i, d: seen_o.append(i))
            got = PF.RKMoire(order=order).sample_model(x0.to(dev), lambda x, t, s, a: x @ wd + x * s, pp, so(), 24, callback=lambda x, i, d: seen_p.append(i))
            assert seen_o == seen_p, (dtype, order, seen_o, seen_p)
            assert got.dtype == dtype and rel_err(got, ref) <= tol, (dtype, order, rel_err(got, ref))
    # the norms themselves
    a, b = torch.randn(3, 1000, generator=g), torch.randn(3, 1000, generator=g)
    assert abs(PF.FunctionalAdaptive.mse(a.to(dev), b.to(dev)) - ((a.double() - b.double()) ** 2).mean().item()) < 1e-12
    assert abs(PF.FunctionalAdaptive.mae(a.to(dev), b.to(dev)) - (a.double() - b.double()).abs().mean().item()) < 1e-12
    assert abs(PF.FunctionalAdaptive.mse(0, b.bfloat16().to(dev)) - (b.bfloat16().double() ** 2).mean().item()) < 1e-12


def test_noise_seeding_rules(dev):
    "reference get_step_noise (diffusers.py:312-346): per-item generators, a single generator for batch 1, else seeds from the data"
    from skrample_amd.pytorch import noise as PN

    def run(shape, generator, x0):
        w = PD.SkrampleWrapperScheduler(PT.Euler(stochasticity=1), PS.Scaled())
        w.set_timesteps(4)
        x = x0
        for t in w.timesteps:
            x = w.step(torch.zeros_like(x0), t, x, generator=generator, return_dict=False)[0]
        return x, w

    g = torch.Generator().manual_seed(18)
    x3 = torch.randn(3, 4, 16, 16, generator=g).to(dev)
    a, w = run(x3.shape, None, x3)  # fallback: one seed per item from its middle element
    b, _ = run(x3.shape, None, x3)
    assert torch.equal(a, b) and len(w._noise_generator.generators) == 3
    c, _ = run(x3.shape, torch.Generator().manual_seed(1), x3)  # a lone generator for a batch of 3 is ignored, as in the reference
    assert torch.equal(a, c)
    d, _ = run(x3.shape, [torch.Generator().manual_seed(s) for s in (1, 2, 3)], x3)
    e, _ = run(x3.shape, [1, 2, 3], x3)  # ints are accepted as seeds
    assert torch.equal(d, e) and not torch.equal(a, d)
    assert not torch.equal(d[0], d[1])  # different seeds, different noise
    x1 = x3[:1].contiguous()
    f, w1 = run(x1.shape, torch.Generator().manual_seed(1), x1)
    assert torch.equal(f, d[:1]) and len(w1._noise_generator.generators) == 1  # same seed, same item => same result


def test_two_streams_do_not_interfere(dev):
    """Every entry point launches on the caller's stream and keeps no per-call state: two sampling loops interleaved on two HIP
    streams (one with in-kernel Philox noise, one with Pyramid noise drawn ahead on its own side stream) give the bits of the
    same loops run one after the other."""
    from skrample_amd.pytorch import noise as PN

    shape, steps = (4, 4, 32, 32), 6
    g = torch.Generator().manual_seed(77)
    xa, xb = (torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(2))
    outs = [torch.randn(shape, generator=g).bfloat16().to(dev) for _ in range(steps)]
    mk_a = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2, stochasticity=1), PS.Karras(PS.Scaled()))  # noqa: E731
    mk_b = lambda: PD.SkrampleWrapperScheduler(PT.UniPC(order=3, stochasticity=1), PS.Scaled(), noise_type=PN.Pyramid)  # noqa: E731

    def alone(mk, x, seeds):
        w = mk()
        w.set_timesteps(steps)
        for i, t in enumerate(w.timesteps.tolist()):
            x = w.step(outs[i], t, x, generator=seeds, return_dict=False)[0]
        torch.cuda.synchronize()
        return x.clone()

    want_a, want_b = alone(mk_a, xa, [1, 2, 3, 4]), alone(mk_b, xb, [5, 6, 7, 8])
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    wa, wb = mk_a(), mk_b()
    wa.set_timesteps(steps)
    wb.set_timesteps(steps)
    ta, tb = wa.timesteps.tolist(), wb.timesteps.tolist()
    torch.cuda.synchronize()
    ya, yb = xa, xb
    for i in range(steps):
        with torch.cuda.stream(sa):
            ya = wa.step(outs[i], ta[i], ya, generator=[1, 2, 3, 4], return_dict=False)[0]
        with torch.cuda.stream(sb):
            yb = wb.step(outs[i], tb[i], yb, generator=[5, 6, 7, 8], return_dict=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(ya, want_a) and torch.equal(yb, want_b)


def test_more_than_two_to_the_31_elements_in_one_launch(dev, fused_mode):
    """Maximum sizes: a single launch over 2^31 + 6144 bf16 elements (4.3 GB per tensor), deterministic and with in-kernel Philox
    noise; every index in the kernels is 64-bit.  Checked on device against torch in fp32, chunk by chunk, around the 2^31 boundary
    and at both ends, plus a whole-tensor checksum; the noise prefix equals the noise of a small launch with the same seed."""
    if torch.cuda.mem_get_info(dev)[0] < 40 * 2**30:
        pytest.skip("needs ~30 GB of free HBM")
    n = 2**31 + 6144
    sched, model = PS.Scaled(), PM.NoiseModel()
    g = torch.Generator(device=dev).manual_seed(123)
    x = torch.empty((1, n), dtype=torch.bfloat16, device=dev)
    out = torch.empty((1, n), dtype=torch.bfloat16, device=dev)
    for t in (x, out):  # filled in slices: one fp32 temporary of 2^31 elements would be 8.6 GB
        for lo in range(0, n, 2**28):
            hi = min(lo + 2**28, n)
            t[0, lo:hi] = torch.randn(hi - lo, device=dev, generator=g)
    step = (0.2, 0.3)
    # the op-tape kernel (the default for a direct call on bf16 tensors) over the same tensors: elementwise, so windows at both ends and
    # across 2^31 must equal small launches on copies of those windows, bit for bit
    from skrample_amd.sampling import native

    native.mode = "auto"
    try:
        whole = PT.DPM(order=1, stochasticity=0).sample(x, out, step, model, sched).final
        for lo in (0, 2**31 - 4096, n - 8192):
            part = PT.DPM(order=1, stochasticity=0).sample(x[:, lo : lo + 8192].contiguous(), out[:, lo : lo + 8192].contiguous(), step, model, sched).final
            assert torch.equal(whole[:, lo : lo + 8192], part), lo
        del whole
    finally:
        native.mode = "never"
    rec = PT.Euler().sample(x, out, step, model, sched)
    got = rec.final
    assert tuple(got.shape) == (1, n) and got.dtype == torch.bfloat16
    small = PT.Euler().sample(x[:, :8192].contiguous(), out[:, :8192].contiguous(), step, model, sched).final
    # the step's two coefficients are recovered from a small launch of the same step (that path is oracle-checked elsewhere);
    # torch then applies them in fp32 to every slice of the large tensors
    xs, os_ = x[0, :8192].float(), out[0, :8192].float()
    sol = torch.linalg.lstsq(torch.stack([xs, os_], dim=1).double(), small[0].double().unsqueeze(1)).solution.flatten()
    c0, c1 = sol.tolist()
    total_got = total_want = 0.0
    for lo in range(0, n, 2**27):
        hi = min(lo + 2**27, n)
        want = (x[0, lo:hi].float() * c0 + out[0, lo:hi].float() * c1)
        diff = (got[0, lo:hi].float() - want).abs()
        tol = want.abs() * 2.0**-7 + 1e-2  # one bf16 rounding of the result (+ the 3-digit recovery of the coefficients)
        assert bool((diff <= tol).all()), (lo, hi, float(diff.max()))
        total_got += float(got[0, lo:hi].double().sum())
        total_want += float(want.double().sum())
    assert abs(total_got - total_want) <= 1e-3 * n**0.5 * 4  # sums of 2e9 values agree to rounding noise
    # in-kernel Philox noise over a sample longer than 2^31 elements
    seeds = torch.tensor([77], dtype=torch.int64, device=dev)
    pn = lazy.PhiloxNoise(seeds, 512, (1, n), dev)
    assert pn.fusable()
    noisy = PT.Euler(stochasticity=1).sample(x, out, step, model, sched, pn).final
    pn_small = lazy.PhiloxNoise(seeds, 512, (1, 2**20), dev)
    noisy_small = PT.Euler(stochasticity=1).sample(x[:, : 2**20].contiguous(), out[:, : 2**20].contiguous(), step, model, sched, pn_small).final
    assert torch.equal(noisy[:, : 2**20], noisy_small)  # element e of a sample draws Philox block e/4 whatever the launch size
    tail = (noisy[0, -(2**22) :].float() - got[0, -(2**22) :].float())  # zeta * N(0,1) up to bf16 rounding
    assert torch.isfinite(noisy[0, 2**31 - 4096 :].float()).all() and abs(float(tail.mean())) < 5e-3 * float(tail.std()) + 1e-3 and float(tail.std()) > 0
