"""Dynamic thresholding on the device: the exact per-sample quantile against numpy in float64, the thresholded step against its definition
and against skr_step_launch over its own stored prediction, the scheduler wrapper against a float64 loop, and the refusals."""

import math

import numpy as np
import pytest
import torch
from test_step_gpu import assert_close

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, graphs, rolling
from skrample_amd.sampling import lazy, models
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
A, B = 1.25, -0.75
ULP = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24}  # half a unit in the last place of a value in [1, 2)


def make_data(kind: str, n: int, dtype, g):
    "(x, o, a, b, ratios) of batch 3: what each data set of the case table is made of"
    x, o, a, b, ratios = torch.randn(3, n, generator=g) * 3, torch.randn(3, n, generator=g) * 3, A, B, [0.995, 0.5, 1.0]
    if kind == "equal":  # every element a candidate
        x, o = torch.full((3, n), 0.75), torch.full((3, n), 0.5)
    elif kind == "two_bins":  # rank k the last 0.5, rank k + 1 the first 4.0: two top-level bins
        low = max(int(0.99 * n), 1) if n > 1 else 1
        x = torch.cat([torch.full((3, low), 0.5), torch.full((3, n - low), 4.0)], dim=1)[:, torch.randperm(n, generator=g)]
        o, a, b, ratios = torch.zeros(3, n), 1.0, 1.0, [(low - 1 + 0.25) / (n - 1), *ratios]
    elif kind == "low_bits":  # x0 = 1 + j 2^-21: values that differ inside their low 10 mantissa bits only
        x, o, a, b = torch.ones(3, n), torch.randint(0, 256, (3, n), generator=g).float(), 1.0, 2.0**-21
    elif kind == "tiny":  # zeros, denormals, both signs
        x, o, a, b = torch.randint(-4, 5, (3, n), generator=g).float() * torch.tensor([1.0, -0.0, 1.0]).reshape(3, 1), torch.zeros(3, n), 1e-40, 1.0
    elif kind == "nan":
        x[1, n // 2] = math.nan
    elif kind == "inf":
        x[0, n // 3] = math.inf
    return x.to(dtype).to(DEV), o.to(dtype).to(DEV), a, b, ratios


def reference_scale(x, o, a, b, ratio, max_value):
    """(s, exact): x0 from three separate numpy float32 operations, np.quantile of |x0| in float64, rounded once; `exact` where w == 0 or
    A[k] == A[k+1].  Where np.quantile's two-sided formula subtracts inf from inf in a sample that holds no NaN, the header's own formula
    A[k] + w (A[k+1] - A[k]) is evaluated in float64 instead."""
    x0 = np.float32(a) * x.float().cpu().numpy() + np.float32(b) * o.float().cpu().numpy()
    assert x0.dtype == np.float32
    mags = np.sort(np.abs(x0).astype(np.float64), axis=1)
    n = mags.shape[1]
    r = ratio * (n - 1)
    k, w = math.floor(r), r - math.floor(r)
    lo, hi = mags[:, k], mags[:, min(k + 1, n - 1)]
    with np.errstate(invalid="ignore"):
        q = np.quantile(mags, ratio, axis=1)
        q = np.where(np.isnan(q) & ~np.isnan(mags).any(axis=1), lo + w * (hi - lo), q)
        s = np.minimum(np.maximum(q.astype(np.float32), np.float32(1.0)), np.float32(max_value))
    s[np.isnan(q)] = np.nan
    return s, (w == 0.0) | (lo == hi)


def device_scale(x, o, a, b, ratio, max_value):
    scale = torch.full((x.shape[0],), -7.0, dtype=torch.float32, device=DEV)
    _hip.launch_threshold_scale(x, o, a, b, ratio, max_value, x.shape[1], scale)
    return scale.cpu().numpy()


@pytest.mark.parametrize("kind", ["normal", "equal", "two_bins", "low_bits", "tiny", "nan", "inf"])
@pytest.mark.parametrize("n", [8, 2048, 2056, 6144, 12288])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_scale_against_float64(dtype, n, kind):
    x, o, a, b, ratios = make_data(kind, n, dtype, torch.Generator().manual_seed(n))
    for ratio in ratios:
        for max_value in (1.5, 1e30):
            got = device_scale(x, o, a, b, ratio, max_value)
            ref, exact = reference_scale(x, o, a, b, ratio, max_value)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            if kind == "nan":
                assert np.isnan(got[1]) and not np.isnan(got[[0, 2]]).any()
            ok = ~np.isnan(ref)
            units = np.abs(got[ok].view(np.int32).astype(np.int64) - ref[ok].view(np.int32).astype(np.int64))
            assert (units <= np.where(exact[ok], 0, 1)).all(), (units, exact)
            alone = device_scale(x[1:2].clone(), o[1:2].clone(), a, b, ratio, max_value)  # the same sample alone, at another address
            assert alone.view(np.int32)[0] == got.view(np.int32)[1]


def plan_for(n_terms, dtype, coefs, zeta=0.0, sample_numel=0, out=True):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n_terms
    plan.dtype_a = plan.dtype_b = _hip.DTYPE_CODE[dtype]
    plan.out0_dtype, plan.out1_dtype = (_hip.DTYPE_CODE[dtype] if out else _hip.NONE), _hip.NONE
    for k, c in enumerate(coefs):
        plan.coef0[k] = c
    if zeta:
        plan.noise_mode, plan.zeta0, plan.stream0, plan.sample_numel = 1, zeta, 5, sample_numel
    return plan


@pytest.mark.parametrize("draw", [False, True], ids=["euler", "dpm2_sde"])
@pytest.mark.parametrize("shape", [(2, 2048), (3, 1000)], ids=["one_trip", "grid_stride"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_step_against_the_definition(dtype, shape, draw):
    g = torch.Generator().manual_seed(shape[1] + draw)
    x, o, h = ((torch.randn(shape, generator=g) * 2).to(dtype).to(DEV) for _ in range(3))
    operands, coefs = ([x, o, h], [0.7, 0.9, -0.4]) if draw else ([x, o], [0.7, 0.5])
    xslot, slot, numel = 0, 1, x.numel()
    seeds = torch.tensor([11, 12, 13][: shape[0]], dtype=torch.int64, device=DEV) if draw else None
    plan = plan_for(len(operands), dtype, coefs, 0.3 if draw else 0.0, shape[1])
    scale = torch.empty(shape[0], dtype=torch.float32, device=DEV)
    _hip.launch_threshold_scale(x, o, A, B, 0.9, 1e30, shape[1], scale)
    s_ref, _ = reference_scale(x, o, A, B, 0.9, 1e30)

    def launch(scale_dev=scale, only=False):
        out, p = (None if only else torch.empty_like(x)), torch.empty_like(x)
        args = (plan_for(2, dtype, [0, 0], out=False), [o, x], None, p, scale_dev, A, B, shape[1], 0, 1, None) if only else (plan, operands, out, p, scale_dev, A, B, shape[1], slot, xslot, seeds)
        _hip.launch_step_thresholded(*args, numel, DEV)
        return out, p

    out, p = launch()
    x0 = (np.float32(A) * x.float().cpu().numpy() + np.float32(B) * o.float().cpu().numpy()).astype(np.float64)
    s64 = s_ref.astype(np.float64).reshape(-1, 1)
    p_ref = np.clip(x0, -s64, s64) / s64
    # the rounding to T (half a unit in the last place of p_ref) plus the one-ulp freedom of s through the division
    bound = ULP[dtype] * 2.0 ** np.floor(np.log2(np.maximum(np.abs(p_ref), 1e-30))) + 2.0**-22 * np.abs(p_ref)
    assert (np.abs(p.double().cpu().numpy() - p_ref) <= bound).all()
    # the step over the launch's own stored prediction, bit for bit
    plain = torch.empty_like(x)
    _hip.launch_step(plan, [p if k == slot else t for k, t in enumerate(operands)], plain, None, seeds, numel, DEV)
    assert torch.equal(out.view(torch.int16 if dtype != torch.float32 else torch.int32), plain.view(torch.int16 if dtype != torch.float32 else torch.int32))
    assert torch.equal(launch(only=True)[1].view(torch.uint8), p.view(torch.uint8))  # the thresholding-only form: the same p
    lib = _hip.load()
    try:
        lib.skr_set_tuning(b"one_trip", 0)  # the grid-stride kernel: the same bits
        out_gs, p_gs = launch()
    finally:
        lib.skr_set_tuning(b"one_trip", 1)
    assert torch.equal(out_gs.view(torch.uint8), out.view(torch.uint8)) and torch.equal(p_gs.view(torch.uint8), p.view(torch.uint8))
    clipped = launch(scale_dev=None)[1]  # no scale: a clip at 1
    assert torch.equal(clipped.cpu(), torch.from_numpy(np.clip(x0, -1.0, 1.0)).to(dtype))


SAMPLERS = {"euler": PT.Euler(), "dpm2_sde": PT.DPM(order=2, stochasticity=1), "adams3": PT.Adams(order=3), "unipc2": PT.UniPC(order=2)}


@pytest.mark.parametrize("shape", [(2, 4, 32, 32), (3, 3, 32, 32)], ids=["whole_chunks", "ragged"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_wrapper_against_the_float64_loop(name, shape):
    "4 bf16 steps under set_thresholding(0.995, 1.5) against numpy thresholding and the same wrapper under DataModel on float64 host tensors"
    steps, ratio, max_value, dtype = 4, 0.995, 1.5, torch.bfloat16
    w = PD.SkrampleWrapperScheduler(SAMPLERS[name], PS.Karras(PS.Scaled()))
    ref = PD.SkrampleWrapperScheduler(SAMPLERS[name], PS.Karras(PS.Scaled()), models.DataModel(), compute_scale=torch.float64)
    w.set_thresholding(ratio, max_value)
    w.set_timesteps(steps), ref.set_timesteps(steps)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(shape, generator=g) * float(w.init_noise_sigma)).to(dtype)
    seeds = list(range(40, 40 + shape[0]))
    noisy = SAMPLERS[name].require_noise
    for i, t in enumerate(w.timesteps):
        out = torch.randn(shape, generator=g).to(dtype)
        a, b = w.model.x_weights(PT._ipoint(w.schedule, i / steps))
        x0 = (np.float32(a) * x.float().numpy() + np.float32(b) * out.float().numpy()).astype(np.float64)
        q = np.quantile(np.abs(x0).reshape(shape[0], -1), ratio, axis=1).astype(np.float32).astype(np.float64)
        s = np.clip(q, 1.0, max_value).reshape(-1, 1, 1, 1)
        p_ref = torch.from_numpy(np.clip(x0, -s, s) / s).to(dtype).double()  # the definition's p is a value of T: what history holds
        gens = [torch.Generator().manual_seed(sd) for sd in seeds] if noisy else None
        got, p = w.step(out.to(DEV), t, x.to(DEV), generator=gens, return_dict=False)
        if noisy:  # the reference steps with the draw the device made
            noise = w._previous[-1].noise
            drawn = (noise.realize(torch.float32) if isinstance(noise, lazy.PhiloxNoise) else noise).double().cpu()
            ref.get_step_noise = lambda *args, drawn=drawn, **kwargs: drawn
        want = ref.step(p_ref, t, x.double(), return_dict=False)[0]
        p = p.materialize() if isinstance(p, lazy.LazyTensor) else p
        assert_close(p, p_ref.to(dtype), dtype, f"{name} p {i}")
        assert_close(got, want.to(dtype), dtype, f"{name} step {i}")  # (the float64 result rounded once, as the existing parity tests hand it over)
        assert not w._raw_outputs or torch.equal(p, w._raw_outputs[-1])  # pred_original_sample is the stored p: what history holds
        x = want.to(dtype)


def test_step_guided_under_thresholding_is_step_on_torchs_guidance_lines():
    shape, dtype = (2, 4, 32, 32), torch.bfloat16
    g = torch.Generator().manual_seed(2)
    x, u, c = ((torch.randn(shape, generator=g)).to(dtype).to(DEV) for _ in range(3))
    results = []
    for guided in (True, False):
        w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
        w.set_thresholding(0.995, 1.5)
        w.set_timesteps(4)
        t = w.timesteps[0]
        results.append(w.step_guided(u, c, 5.0, t, x, return_dict=False) if guided else w.step(u + 5.0 * (c - u), t, x, return_dict=False))
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_refusals_name_thresholding():
    x = torch.randn(2, 4, 32, 32, device=DEV).bfloat16()

    def wrapper(**kw):
        w = PD.SkrampleWrapperScheduler(PT.Euler(), PS.Karras(PS.Scaled()), **kw)
        w.set_thresholding(0.995, 1.5)
        w.set_timesteps(4)
        return w

    w = wrapper()
    with pytest.raises(lazy.SkrampleHipError, match="thresholding"):
        w.set_inpaint(torch.ones(32, 32, device=DEV), x, x)
    with pytest.raises(lazy.SkrampleHipError, match="thresholding"):
        wrapper(compute_scale=None).step(x.clone(), w.timesteps[0], x)
    with pytest.raises(lazy.SkrampleHipError, match="thresholding"):
        w.step(x.float().requires_grad_().bfloat16(), w.timesteps[0], x)
    with pytest.raises(lazy.SkrampleHipError, match="thresholding"):
        w.step(x.double(), w.timesteps[0], x.double())
    with pytest.raises(lazy.SkrampleHipError, match="thresholding"):
        graphs.capture_sampling_loop(w, lambda s, t: s, x, 4)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(lazy.SkrampleHipError, match="thresholding"):
        rolling.RollingBatch(wrapper, x, capacity=2)
    assert torch.cuda.memory_allocated(DEV) == before  # a refused batch allocates nothing
    # non-contiguous operands are copied, as on the general path
    y = torch.randn(2, 4, 32, 64, device=DEV).bfloat16()[..., ::2]
    assert torch.equal(wrapper().step(y, w.timesteps[0], x, return_dict=False)[0], wrapper().step(y.contiguous(), w.timesteps[0], x, return_dict=False)[0])
