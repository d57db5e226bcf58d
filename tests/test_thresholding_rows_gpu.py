"""Dynamic thresholding with device-resident rows (needs an MI355X): skr_threshold_scale_indexed[_per_sample] and
skr_thresholded_step_launch_indexed[_per_sample] through the C ABI against numpy in float64 and against the direct entries on each sample
alone, `capture_sampling_loop(..., thresholded=True)` against the eager thresholded loop, and the statistic's stores inside an arena."""

import ctypes
import math

import numpy as np
import pytest
import torch
from arena import Arena, untouched
from test_thresholding_gpu import make_data, plan_for, reference_scale

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
ULP = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11, torch.float32: 2.0**-24}  # half a unit in the last place of a value in [1, 2)
dtype_id = lambda d: str(d).split(".")[1]  # noqa: E731
bits = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731


def row_of(a, b, ratio, max_value, coefs=(), zeta=0.0, stream=0):
    row = _hip.StepRowC()
    for k, c in enumerate(coefs):
        row.coef0[k] = c
    row.zeta0, row.stream0 = zeta, stream
    row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3] = a, b, ratio, max_value
    return row


def table_of(rows):
    "the rows behind one row of 0xFF bytes (every launch below passes row_offset = 1), and an int32 index vector to fill"
    tab = torch.full(((len(rows) + 1) * ctypes.sizeof(_hip.StepRowC),), 0xFF, dtype=torch.uint8, device=DEV)
    _hip.upload_rows(tab, 1, rows)
    return tab


def index_of(entries):
    return torch.tensor(entries, dtype=torch.int32, device=DEV)


def scale_rows(x, o, tab, index, scale, workspace, per_sample):
    entry = getattr(_hip.load(), "skr_threshold_scale_indexed" + ("_per_sample" if per_sample else ""))
    status = entry(x.data_ptr(), o.data_ptr(), _hip.DTYPE_CODE[x.dtype], x.numel(), x.shape[1], tab.data_ptr(), index.data_ptr(), 1, scale.data_ptr(), workspace.data_ptr(),
                   _hip.current_stream_ptr(DEV))  # fmt: skip
    assert status == 0, status


def direct_scale(x, o, a, b, ratio, max_value):
    scale = torch.empty(x.shape[0], dtype=torch.float32, device=DEV)
    _hip.launch_threshold_scale(x, o, a, b, ratio, max_value, x.shape[1], scale)
    return scale


@pytest.mark.parametrize("kind", ["normal", "equal", "two_bins", "nan"])
@pytest.mark.parametrize("n", [2048, 6144])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_scale_rows_against_float64(dtype, n, kind):
    """three rows for three samples through the per-sample entry (the third a plain-clip row: its slot keeps the poison), then index_dev
    moved between two resident rows through the indexed entry; test_scale_against_float64's bar, and the direct entry's bits"""
    x, o, a, b, ratios = make_data(kind, n, dtype, torch.Generator().manual_seed(n))
    settings = [(a, b, ratios[0], 1.5), (0.5 * a, 2.0 * b, ratios[1], 1e30), (a, b, ratios[0], 1.0)]
    tab = table_of([row_of(*s) for s in settings])
    workspace = torch.empty(_hip.threshold_workspace(3 * n, n), dtype=torch.uint8, device=DEV)

    def check(got, s, setting):
        ref, exact = reference_scale(x[s : s + 1], o[s : s + 1], *setting)
        assert np.isnan(got) == np.isnan(ref[0]) and (kind != "nan" or np.isnan(got) == (s == 1))
        if not np.isnan(got):
            units = abs(int(np.float32(got).view(np.int32)) - int(ref.view(np.int32)[0]))
            assert units <= (0 if exact[0] else 1), (units, exact)
        alone = direct_scale(x[s : s + 1].clone(), o[s : s + 1].clone(), *setting).cpu().numpy()  # the same sample alone, at another address
        assert alone.view(np.int32)[0] == np.float32(got).view(np.int32)

    scale = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    assigned = [1, 0, 2]
    scale_rows(x, o, tab, index_of(assigned), scale, workspace, True)
    got = scale.cpu().numpy()
    assert got[2] == -7.0  # the plain-clip row's sample: never written
    for s in (0, 1):
        check(got[s], s, settings[assigned[s]])
    index = index_of([0])
    for at in (0, 1, 0):
        index.fill_(at)
        scale.fill_(-7.0)
        scale_rows(x, o, tab, index, scale, workspace, False)
        got = scale.cpu().numpy()
        for s in range(3):
            check(got[s], s, settings[at])
    index.fill_(2)
    scale.fill_(-7.0)
    scale_rows(x, o, tab, index, scale, workspace, False)
    assert (scale == -7.0).all()  # a plain-clip row for the whole batch: the launch writes nothing


FORMS = {"only": (2, [0.0, 0.0], False), "euler": (2, [0.7, 0.5], False), "dpm2_sde": (3, [0.7, 0.9, -0.4], True)}


@pytest.mark.parametrize("per_sample", [False, True], ids=["indexed", "per_sample"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
def test_step_rows(dtype, form, per_sample):
    """statistics row launch, then row step, over (3, 2048): p against the float64 definition, `out` and p bit-equal to the direct launches on
    each sample alone with its row's values; the plain-clip row (zeta 0 too: no draw) equals scale_dev=None, its NaN scale slot unread"""
    n_ops, coefs, draws = FORMS[form]
    only, n = form == "only", 2048
    g = torch.Generator().manual_seed(n_ops + 10 * draws)
    x, o, h = ((torch.randn((3, n), generator=g) * 2).to(dtype).to(DEV) for _ in range(3))
    operands, slot, xslot = ([o, x], 0, 1) if only else ([x, o, h][:n_ops], 1, 0)
    seeds = torch.tensor([11, 12, 13], dtype=torch.int64, device=DEV) if draws else None
    settings = [(1.25, -0.75, 0.9, 1e30), (0.8, -1.1, 0.5, 1.5), (1.25, -0.75, 0.9, 1.0)]
    steps = [(coefs, 0.3 if draws else 0.0, 5), ([c * 0.5 for c in coefs], 0.2 if draws else 0.0, 9), ([c + 0.25 for c in coefs], 0.0, 7)]
    tab = table_of([row_of(*s, *st) for s, st in zip(settings, steps)])
    assigned = [0, 1, 2] if per_sample else [1, 1, 1]
    index = index_of(assigned if per_sample else [1])
    scale = torch.full((3,), math.nan, dtype=torch.float32, device=DEV)
    scale_rows(x, o, tab, index, scale, torch.empty(_hip.threshold_workspace(3 * n, n), dtype=torch.uint8, device=DEV), per_sample)
    plan = plan_for(n_ops, dtype, [0.0] * n_ops, 1.0 if draws else 0.0, n, out=not only)  # (the plan's scalars are not the rows')
    out, p = (None if only else torch.empty_like(x)), torch.empty_like(x)
    thr = _hip.StepThresholdC(scale.data_ptr(), p.data_ptr(), 0.0, 0.0, n, slot, xslot, 0)
    entry = getattr(_hip.load(), "skr_thresholded_step_launch_indexed" + ("_per_sample" if per_sample else ""))
    status = entry(ctypes.byref(plan), _hip._operand_array(operands), _hip._ptr(out), ctypes.byref(thr), _hip._ptr(seeds), x.numel(), tab.data_ptr(), index.data_ptr(), 1,
                   _hip.current_stream_ptr(DEV))  # fmt: skip
    assert status == 0, status
    for s, at in enumerate(assigned):
        (a, b, ratio, max_value), (c, zeta, stream) = settings[at], steps[at]
        lone = [t[s : s + 1].clone() for t in operands]
        lone_scale = direct_scale(lone[xslot], lone[slot], a, b, ratio, max_value) if max_value > 1.0 else None
        lone_plan = plan_for(n_ops, dtype, c, zeta, n, out=not only)
        lone_plan.stream0 = stream
        want_out, want_p = (None if only else torch.empty_like(lone[0])), torch.empty_like(lone[0])
        _hip.launch_step_thresholded(lone_plan, lone, want_out, want_p, lone_scale, a, b, n, slot, xslot, seeds[s : s + 1].clone() if draws else None, n, DEV)
        assert torch.equal(bits(p[s]), bits(want_p[0])) and (only or torch.equal(bits(out[s]), bits(want_out[0]))), (s, at)
        s_ref = reference_scale(lone[xslot], lone[slot], a, b, ratio, max_value)[0].astype(np.float64) if max_value > 1.0 else np.ones(1)
        x0 = (np.float32(a) * lone[xslot].float().cpu().numpy() + np.float32(b) * lone[slot].float().cpu().numpy()).astype(np.float64)
        p_ref = np.clip(x0, -s_ref[0], s_ref[0]) / s_ref[0]
        # the rounding to T (half a unit in the last place of p_ref) plus the one-ulp freedom of s through the division
        bound = ULP[dtype] * 2.0 ** np.floor(np.log2(np.maximum(np.abs(p_ref), 1e-30))) + 2.0**-22 * np.abs(p_ref)
        assert (np.abs(p[s : s + 1].double().cpu().numpy() - p_ref) <= bound).all()


# ---- captured loops ------------------------------------------------------------------------------------------------------------------
SAMPLERS = {"euler": PT.Euler, "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1), "unipc2": lambda: PT.UniPC(order=2)}
SCHEDULES = [lambda: PS.Karras(PS.Scaled()), lambda: PS.Exponential(PS.Scaled())]
SETTINGS = [(0.995, 1.5), (0.9, 3.0)]
STEPS, SEEDS, LATENTS = 4, [40, 41], (2, 4, 32, 32)


def net(x, t):
    return x * 0.5 + 0.3 * x.abs()


def wrapper_of(name, which=0, setting=None, **fields):
    w = PD.SkrampleWrapperScheduler(SAMPLERS[name](), SCHEDULES[which](), **fields)
    w.set_thresholding(*(setting or SETTINGS[which]))
    return w


def eager(w, x, seeds=SEEDS):
    w.set_timesteps(STEPS)
    for t in w.timesteps.tolist():
        x = w.step(net(x, t), t, x, generator=list(seeds), return_dict=False)[0]
    return x.clone()


@pytest.fixture(scope="module")
def x0():
    w = wrapper_of("euler")
    return (torch.randn(LATENTS, generator=torch.Generator().manual_seed(41)) * float(w.init_noise_sigma)).bfloat16().to(DEV)


@pytest.fixture(scope="module")
def eager_runs(x0):
    "{(sampler, which): the eager thresholded loop}, and which = 2: schedule 0 under a plain clip; computed once and shared"
    runs = {(name, which): eager(wrapper_of(name, which), x0) for name in SAMPLERS for which in (0, 1)}
    runs.update({(name, 2): eager(wrapper_of(name, 0, (0.995, 1.0)), x0) for name in SAMPLERS})
    return runs


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_captured_thresholded_loop(name, x0, eager_runs):
    """indexed=False, indexed=True and per_sample=True replays equal the eager thresholded loop bit for bit; after retarget to another schedule
    and another (ratio, max) -- and to a plain clip -- the replay equals that wrapper's eager loop; two samples on two wrappers equal their runs"""
    frozen = capture_sampling_loop(wrapper_of(name), net, x0, STEPS, seeds=SEEDS, thresholded=True)
    assert frozen.rows is None and torch.equal(bits(frozen(x0)), bits(eager_runs[(name, 0)])), name
    loop = capture_sampling_loop(wrapper_of(name), net, x0, STEPS, seeds=SEEDS, indexed=True, thresholded=True)
    assert loop.thresholded and loop.rows.scale.shape == (2,) and [tuple(r.convert_k)[2:] for r in loop.rows.host[:1]] == [SETTINGS[0]]
    loop.retarget(wrapper_of(name, 1), slot=1)
    loop.retarget(wrapper_of(name, 0, (0.995, 1.0)), slot=2)
    for which in (0, 1, 2, 0):
        assert torch.equal(bits(loop(x0, slot=which)), bits(eager_runs[(name, which)])), (name, which)
    assert not torch.equal(eager_runs[(name, 0)], eager_runs[(name, 1)]) and not torch.equal(eager_runs[(name, 0)], eager_runs[(name, 2)])
    each = capture_sampling_loop(wrapper_of(name), net, x0, STEPS, seeds=SEEDS, indexed=True, per_sample=True, thresholded=True)
    assert torch.equal(bits(each(x0)), bits(eager_runs[(name, 0)])), name
    each.retarget(wrapper_of(name, 1), slot=1)
    each.retarget(wrapper_of(name, 0, (0.995, 1.0)), slot=2)
    for slots in ([0, 1], [2, 0]):
        got = each(x0, slot=slots)
        for s, which in enumerate(slots):  # sample s of the eager whole-batch run of its wrapper: a sample's bits do not depend on its neighbours
            assert torch.equal(bits(got[s]), bits(eager_runs[(name, which)][s])), (name, slots, s)


def test_what_stays_refused(x0):
    "one case for each combination left refused, each under its reason"
    with pytest.raises(_hip.SkrampleHipError, match="thresholded=True"):
        capture_sampling_loop(wrapper_of("euler"), net, x0, STEPS, indexed=True)
    with pytest.raises(ValueError, match="set_thresholding"):
        capture_sampling_loop(PD.SkrampleWrapperScheduler(PT.Euler(), SCHEDULES[0]()), net, x0, STEPS, thresholded=True)
    with pytest.raises(_hip.SkrampleHipError, match="guidance-only launch has no row form"):
        capture_sampling_loop(wrapper_of("euler"), lambda x, t: (net(x, t), x * 0.25), x0, STEPS, indexed=True, thresholded=True, guidance_scale=3.0)
    guided = capture_sampling_loop(wrapper_of("euler"), lambda x, t: (net(x, t), x * 0.25), x0, STEPS, thresholded=True, guidance_scale=3.0)
    assert guided(x0).isfinite().all()  # (indexed=False captures it)
    w = wrapper_of("euler")
    with pytest.raises(_hip.SkrampleHipError, match="thresholding"):
        w.set_inpaint(torch.ones(32, 32, device=DEV), x0, x0)
    with pytest.raises(_hip.SkrampleHipError, match="compute_scale=None"):
        capture_sampling_loop(wrapper_of("euler", compute_scale=None), net, x0, STEPS, indexed=True, thresholded=True)
    with pytest.raises(_hip.SkrampleHipError, match="fp64"):
        capture_sampling_loop(wrapper_of("euler"), net, x0.double(), STEPS, indexed=True, thresholded=True)
    with pytest.raises(_hip.SkrampleHipError, match="no backward"):
        capture_sampling_loop(wrapper_of("euler"), net, x0.float().requires_grad_(), STEPS, indexed=True, thresholded=True)
    with pytest.raises(_hip.SkrampleHipError, match="ragged samples have no thresholded row form"):
        capture_sampling_loop(wrapper_of("euler"), net, x0[:, :3].contiguous(), STEPS, indexed=True, thresholded=True)
    loop = capture_sampling_loop(wrapper_of("euler"), net, x0, STEPS, indexed=True, thresholded=True)
    with pytest.raises(ValueError, match="set_thresholding"):
        loop.retarget(PD.SkrampleWrapperScheduler(PT.Euler(), SCHEDULES[1]()), slot=1)


def test_statistic_stays_inside_its_buffers():
    "the per-sample statistic on arena views of exactly SKR_THRESHOLD_WORKSPACE bytes: bands untouched, the plain-clip sample's bytes untouched"
    n, dtype = 6144, torch.bfloat16
    x, o, a, b, ratios = make_data("normal", n, dtype, torch.Generator().manual_seed(7))
    arena = Arena(DEV)
    workspace, scale = arena.take("workspace", _hip.threshold_workspace(3 * n, n), torch.uint8), arena.take("scale", 3, torch.float32)
    tab = table_of([row_of(a, b, ratios[0], 1.5), row_of(a, b, ratios[1], 1.0)])
    scale_rows(x, o, tab, index_of([0, 1, 0]), scale, workspace, True)
    torch.cuda.synchronize()
    arena.check()
    hist, meta, candidates = workspace[: 3 * 8192].view(3, 8192), workspace[3 * 8192 : 3 * 8208].view(3, 16), workspace[3 * 8208 :].view(3, 4 * n)
    assert untouched(scale[1:2]) and untouched(hist[1]) and untouched(meta[1]) and untouched(candidates[1])
    assert not untouched(scale[0:1]) and not untouched(scale[2:3]) and not untouched(hist[0]) and not untouched(hist[2])
    assert scale[0].item() == direct_scale(x[:1], o[:1], a, b, ratios[0], 1.5).item()
