"""Guided dynamic thresholding on the device: skr_guided_threshold_scale and skr_guided_thresholded_step_launch against the two-launch
route (the guidance-only launch, then skr_threshold_scale / skr_thresholded_step_launch over its tensor) bit for bit and against float64,
the wrapper under set_thresholding(..., fuse_guidance=True) against the default route, and a captured fused loop."""

import ctypes

import numpy as np
import pytest
import torch
from test_thresholding_gpu import DEV, DTYPES, SAMPLERS, ULP, A, B, device_scale, make_data, plan_for, reference_scale

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, graphs
from skrample_amd.sampling import lazy

pytestmark = pytest.mark.gpu
G = 7.3
PLANT = 0.1416015625  # fp16: G * PLANT rounds to 0x3c23 once (torch's tail) and to 0x3c22 through fp32 (whole blocks)
ids = lambda d: str(d).split(".")[1]  # noqa: E731


def bits(t):
    return t.contiguous().view(torch.uint8)


def guided_tensor(u, c):
    return lazy.guide_only(lazy.Guidance(u, c, G))


def guided_scale(x, u, c, a, b, ratio, max_value):
    scale = torch.full((x.shape[0],), -7.0, dtype=torch.float32, device=DEV)
    _hip.launch_guided_threshold_scale(x, u, c, G, a, b, ratio, max_value, x.shape[1], scale)
    return scale.cpu().numpy()


@pytest.mark.parametrize("kind", ["normal", "equal", "nan"])
@pytest.mark.parametrize("n", [8, 2048, 2056, 6144])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_scale_is_the_two_launch_scale(dtype, n, kind):
    g = torch.Generator().manual_seed(n)
    x, u, a, b, ratios = make_data(kind, n, dtype, g)
    c = torch.full_like(u, 0.25) if kind == "equal" else torch.randn(3, n, generator=g).to(dtype).to(DEV)
    pg = guided_tensor(u, c)
    for ratio in ratios:
        for max_value in (1.5, 1e30):
            got = guided_scale(x, u, c, a, b, ratio, max_value)
            assert np.array_equal(got.view(np.int32), device_scale(x, pg, a, b, ratio, max_value).view(np.int32))  # (a)
            ref, exact = reference_scale(x, pg, a, b, ratio, max_value)  # (b)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            ok = ~np.isnan(ref)
            units = np.abs(got[ok].view(np.int32).astype(np.int64) - ref[ok].view(np.int32).astype(np.int64))
            assert (units <= np.where(exact[ok], 0, 1)).all(), (units, exact)
            alone = guided_scale(x[1:2].clone(), u[1:2].clone(), c[1:2].clone(), a, b, ratio, max_value)  # (c)
            assert alone.view(np.int32)[0] == got.view(np.int32)[1]


def test_scale_keeps_torchs_fp16_tail_inside_a_whole_aligned_span():
    "3 x 2056 fp16: the last sample's first span is whole and aligned and straddles the tail (6144); its maximum sits in the tail"
    g = torch.Generator().manual_seed(5)
    x, u, c = (((torch.rand(3, 2056, generator=g) - 0.5) * 0.1).half().to(DEV) for _ in range(3))
    for t, v in ((x, 0.0), (u, 0.0), (c, PLANT)):
        t.view(-1)[-24:] = v
    got = guided_scale(x, u, c, 1.0, 1.0, 1.0, 1e30)
    assert got[2] == 1.0341796875 and (got[:2] == 1.0).all()  # (1.033203125 for a kernel that rounds G * PLANT twice there)
    assert np.array_equal(got.view(np.int32), device_scale(x, guided_tensor(u, c), 1.0, 1.0, 1.0, 1e30).view(np.int32))


@pytest.mark.parametrize("draw", [False, True], ids=["euler", "dpm2_sde"])
@pytest.mark.parametrize("shape", [(2, 2048), (3, 1000)], ids=["one_trip", "grid_stride"])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_step_is_the_two_launch_step(dtype, shape, draw):
    g = torch.Generator().manual_seed(shape[1] + draw)
    x, u, c, h = ((torch.randn(shape, generator=g) * 2).to(dtype).to(DEV) for _ in range(4))
    if dtype == torch.float16 and shape == (3, 1000):  # the planted product in a whole block and in torch's tail (index >= 2048)
        for at in (100, 2500):
            u.view(-1)[at], c.view(-1)[at] = 0.0, PLANT
    pg = guided_tensor(u, c)
    operands, coefs = ([x, u, h], [0.7, 0.9, -0.4]) if draw else ([x, u], [0.7, 0.5])
    xslot, slot, numel = 0, 1, x.numel()
    seeds = torch.tensor([11, 12, 13][: shape[0]], dtype=torch.int64, device=DEV) if draw else None
    plan = plan_for(len(operands), dtype, coefs, 0.3 if draw else 0.0, shape[1])
    scale = torch.empty(shape[0], dtype=torch.float32, device=DEV)
    _hip.launch_guided_threshold_scale(x, u, c, G, A, B, 0.9, 1e30, shape[1], scale)

    def launch(scale_dev=scale, only=False):
        out, p = (None if only else torch.empty_like(x)), torch.empty_like(x)
        args = (plan_for(2, dtype, [0, 0], out=False), [u, x], None, p, c, G, scale_dev, A, B, shape[1], 0, 1, None) if only else (
            plan, operands, out, p, c, G, scale_dev, A, B, shape[1], slot, xslot, seeds)  # fmt: skip
        _hip.launch_guided_step_thresholded(*args, numel, DEV)
        return out, p

    out, p = launch()
    out2, p2 = torch.empty_like(x), torch.empty_like(x)
    _hip.launch_step_thresholded(plan, [pg if k == slot else t for k, t in enumerate(operands)], out2, p2, scale, A, B, shape[1], slot, xslot, seeds, numel, DEV)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(p), bits(p2))
    s_ref, _ = reference_scale(x, pg, A, B, 0.9, 1e30)
    x0 = (np.float32(A) * x.float().cpu().numpy() + np.float32(B) * pg.float().cpu().numpy()).astype(np.float64)
    s64 = s_ref.astype(np.float64).reshape(-1, 1)
    p_ref = np.clip(x0, -s64, s64) / s64
    # half a unit in the last place of T at p_ref -- below T's smallest normal the unit stops shrinking (fp16: |p| < 2^-14 occurs here, x0
    # spans +-40) -- plus the one-ulp freedom of s through the division
    binade = np.maximum(np.floor(np.log2(np.maximum(np.abs(p_ref), 1e-30))), -14 if dtype == torch.float16 else -126)
    bound = ULP[dtype] * 2.0**binade + 2.0**-22 * np.abs(p_ref)
    over = np.abs(p.double().cpu().numpy() - p_ref) > bound
    assert not over.any(), (p.double().cpu().numpy()[over], p_ref[over], bound[over])
    assert torch.equal(bits(launch(only=True)[1]), bits(p))  # the thresholding-only form: the same p
    lib = _hip.load()
    try:
        lib.skr_set_tuning(b"one_trip", 0)  # the grid-stride kernel: the same bits
        out_gs, p_gs = launch()
    finally:
        lib.skr_set_tuning(b"one_trip", 1)
    assert torch.equal(bits(out_gs), bits(out)) and torch.equal(bits(p_gs), bits(p))
    assert torch.equal(launch(scale_dev=None)[1].cpu(), torch.from_numpy(np.clip(x0, -1.0, 1.0)).to(dtype))  # no scale: a clip at 1
    # the two refusals of the guidance descriptor: their codes, and nothing written
    kept, arr = torch.full_like(x, 3.0), (ctypes.c_void_p * len(operands))(*(t.data_ptr() for t in operands))
    thr = _hip.StepThresholdC(scale.data_ptr(), kept.data_ptr(), A, B, shape[1], slot, xslot, 0)
    for guide, code in ((_hip.StepGuidanceC(c.data_ptr(), kept.data_ptr(), G, slot, 0), 7), (_hip.StepGuidanceC(c.data_ptr(), None, G, xslot, 0), 3)):
        status = lib.skr_guided_thresholded_step_launch(ctypes.byref(plan), arr, kept.data_ptr(), ctypes.byref(guide), ctypes.byref(thr), seeds.data_ptr() if draw else None, numel, None)
        assert status == code and (kept == 3.0).all()


def fused_and_default(name, shape, dtype, monkeypatch, rescale=0.0, strided=False, steps=4):
    "per step (prev_sample, pred_original_sample) of the fused wrapper and of the default one, and the fused wrapper's guide_only calls"
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(shape, generator=g).to(dtype).to(DEV)
    halves = [torch.randn((2, *shape[:-1], shape[-1] * (2 if strided else 1)), generator=g).to(dtype).to(DEV) for _ in range(steps)]
    runs, calls = [], []
    for fuse in (True, False):
        w = PD.SkrampleWrapperScheduler(SAMPLERS[name], PS.Karras(PS.Scaled()))
        w.set_thresholding(0.995, 1.5, fuse_guidance=True) if fuse else w.set_thresholding(0.995, 1.5)
        w.set_timesteps(steps)
        real, x, got = lazy.guide_only, x0 * float(w.init_noise_sigma), []
        if fuse:
            monkeypatch.setattr(lazy, "guide_only", lambda gd: (calls.append(1), real(gd))[1])
        for t, uc in zip(w.timesteps, halves):
            u, c = (uc[0][..., ::2].contiguous(), uc[1][..., ::2]) if strided else (uc[0], uc[1])
            gens = [torch.Generator().manual_seed(40 + k) for k in range(shape[0])] if SAMPLERS[name].require_noise else None
            x, p = w.step_guided(u, c, 5.0, t, x, generator=gens, return_dict=False, guidance_rescale=rescale)
            got.append((x, p.materialize() if isinstance(p, lazy.LazyTensor) else p))
        monkeypatch.setattr(lazy, "guide_only", real)
        runs.append(got)
    return runs[0], runs[1], len(calls)


@pytest.mark.parametrize("shape,dtype", [((2, 4, 32, 32), torch.bfloat16), ((3, 3, 32, 32), torch.bfloat16), ((3, 3, 32, 32), torch.float16)], ids=["whole", "ragged", "ragged_fp16"])
@pytest.mark.parametrize("name", list(SAMPLERS))
def test_wrapper_fused_route_has_the_default_routes_bits(name, shape, dtype, monkeypatch):
    fused, default, calls = fused_and_default(name, shape, dtype, monkeypatch)
    assert calls == 0
    for (xa, pa), (xb, pb) in zip(fused, default):
        assert torch.equal(bits(xa), bits(xb)) and torch.equal(bits(pa), bits(pb))


@pytest.mark.parametrize("how", [{"rescale": 0.7}, {"strided": True}], ids=["rescaled", "strided_cond"])
def test_wrapper_keeps_the_default_route_where_the_fused_one_does_not_apply(how, monkeypatch):
    fused, default, calls = fused_and_default("dpm2_sde", (2, 4, 32, 32), torch.bfloat16, monkeypatch, **how)
    assert calls > 0
    for (xa, pa), (xb, pb) in zip(fused, default):
        assert torch.equal(bits(xa), bits(xb)) and torch.equal(bits(pa), bits(pb))


def test_captured_fused_loop_replays_the_eager_fused_loop():
    shape, steps, seeds = (2, 4, 32, 32), 4, [40, 41]
    x0 = torch.randn(shape, generator=torch.Generator().manual_seed(9)).bfloat16().to(DEV)
    net = lambda x, t: (x * 0.5, x * 0.25 + 0.125)  # noqa: E731

    def wrapper():
        w = PD.SkrampleWrapperScheduler(SAMPLERS["dpm2_sde"], PS.Karras(PS.Scaled()))
        w.set_thresholding(0.995, 1.5, fuse_guidance=True)
        return w

    w = wrapper()
    w.set_timesteps(steps)
    x = x0
    for t in w.timesteps.tolist():
        u, c = net(x, t)
        x = w.step_guided(u, c, 5.0, t, x, generator=list(seeds), return_dict=False)[0]
    loop = graphs.capture_sampling_loop(wrapper(), net, x0, steps, seeds=seeds, thresholded=True, guidance_scale=5.0)
    for _ in range(3):
        assert torch.equal(bits(loop(x0)), bits(x))
    with pytest.raises(_hip.SkrampleHipError, match="guidance-only launch has no row form"):
        graphs.capture_sampling_loop(wrapper(), net, x0, steps, seeds=seeds, indexed=True, thresholded=True, guidance_scale=5.0)
