"""Adaptive projected guidance on the device, through the C ABI: skr_projected_guidance_coef against the float32 / float64 restatement of
the definition (test_projected_guidance_host), skr_projected_guided_step_launch against that restatement over the device's coefficients
and against skr_step_launch over the stored prediction, and the wrapper under set_projected_guidance against a twin's plain step()."""

import numpy as np
import pytest
import torch
from test_projected_guidance_host import coefficients64, restate_d, restate_p
from test_thresholding_gpu import DEV, DTYPES, ULP, plan_for

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
G = 7.5
SIZES = [2048, 4096, 2056, 520]  # one span, two spans (the stage-2 order), a partial last span, below one span; the first two take the one-trip step
ids = lambda d: str(d).split(".")[1]  # noqa: E731


def bits(t):
    return t.contiguous().view(torch.uint8)


def make(n, dtype, beta, seed):
    "(u, c, m, r) on the CPU, batch 3: sample 1's cond has four times the spread, r lies between the norms of samples 0 and 1, 1 % clear of all three"
    g = torch.Generator().manual_seed(seed)
    u, c, m = (torch.randn(3, n, generator=g) for _ in range(3))
    c[1] *= 4
    u, c, m = u.to(dtype), c.to(dtype), (m * 0.5).to(dtype)
    norms = restate_d(u, c, m, beta).double().pow(2).sum(1).sqrt()
    r = float((norms[0] * norms[1]).sqrt())
    assert norms[0] < r < norms[1] and ((norms - r).abs() > 0.01 * r).all()
    return u, c, m, r


def device_coef(u, c, m, eta, r, beta, stats=False):
    "(coef [samples, 2], the buffer after the launch, stats [samples, 3] or None) of one statistics launch over device copies"
    u, c, m = u.to(DEV), c.to(DEV), m.to(DEV)
    n = u.shape[1]
    coef = torch.full((2 * u.shape[0],), -7.0, dtype=torch.float32, device=DEV)
    partials = torch.empty(_hip.projected_partials(u.numel(), n), dtype=torch.float64, device=DEV)
    sums = torch.empty(3 * u.shape[0], dtype=torch.float64, device=DEV) if stats else None
    _hip.launch_projected_coef(u, c, m, G, eta, r, beta, n, coef, partials, sums)
    return coef.reshape(-1, 2), m, sums.reshape(-1, 3).cpu() if stats else None


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("beta", [0.0, -0.5])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_statistic(dtype, n, beta, eta):
    u, c, m, r = make(n, dtype, beta, n)
    coef, m_after, sums = device_coef(u, c, m, eta, r, beta, stats=True)
    d = restate_d(u, c, m, beta)
    assert torch.equal(bits(m_after.cpu()), bits(d))
    a_ref, b_ref, (sdd, sdc, scc, sadc) = coefficients64(d, c, G, eta, r)
    for k, (ref, terms) in enumerate(((sdd, sdd), (sdc, sadc), (scc, scc))):  # exact products: only the n additions round
        assert ((sums[:, k] - ref).abs() <= n * 2.0**-52 * terms).all(), (k, sums[:, k], ref)
    a, b = coef[:, 0].cpu().double(), coef[:, 1].cpu().double()
    assert ((a - a_ref).abs() <= 2.0**-23 * a_ref.abs()).all(), (a, a_ref)
    assert ((b - b_ref).abs() <= 2.0**-23 * b_ref.abs() + 1e-9 * (a_ref * (1 - eta)).abs() * sadc / scc).all(), (b, b_ref)
    assert a[0] == np.float32(G - 1) and a[1] < a[0]  # sample 0 below the threshold, sample 1 clamped
    alone = device_coef(u[2:3], c[2:3], m[2:3], eta, r, beta)[0]
    assert torch.equal(bits(alone[0]), bits(coef[2]))
    if eta == 1.0:  # no clamp, the parallel part kept: plain guidance
        plain = device_coef(u, c, m, 1.0, 0.0, beta)[0].cpu()
        assert (plain[:, 0] == np.float32(G - 1)).all() and (plain[:, 1] == 1.0).all()


@pytest.mark.parametrize("momentum", [False, True], ids=["registers", "diff"])
@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("last", [False, True], ids=["slot0", "slot_last"])
@pytest.mark.parametrize("K", [2, 6, 13])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_step(dtype, K, last, noise, momentum):
    lib, slot, beta = _hip.load(), (K - 1 if last else 0), (-0.5 if momentum else 0.0)
    for n in SIZES:
        u, c, m, r = make(n, dtype, beta, n + K)
        coef, m_after, _ = device_coef(u, c, m, 0.0, r, beta)
        diff = m_after if momentum else None
        g = torch.Generator().manual_seed(K)
        operands = [torch.randn(3, n, generator=g).to(dtype).to(DEV) for _ in range(K)]
        operands[slot] = u.to(DEV)
        cd, numel = c.to(DEV), 3 * n
        plan = plan_for(K, dtype, [0.9 - 0.17 * k for k in range(K)], 0.3 if noise else 0.0, n)
        seeds = torch.tensor([11, 12, 13], dtype=torch.int64, device=DEV) if noise else None

        def launch(only=False):
            out, p = (None if only else torch.empty_like(cd)), torch.empty_like(cd)
            args = (plan_for(1, dtype, [1.0], out=False), [operands[slot]], None, cd, p, 0) if only else (plan, operands, out, cd, p, slot)
            _hip.launch_projected_guided_step(*args, coef.reshape(-1), diff, n, None if only else seeds, numel, DEV)
            return out, p

        out, p = launch()
        d = restate_d(u, c, m, beta)
        assert torch.equal(bits(p.cpu()), bits(restate_p(c, d, coef[:, 0].cpu(), coef[:, 1].cpu())))
        a64, b64, _ = coefficients64(d, c, G, 0.0, r)
        bc, ad = b64[:, None] * c.double(), a64[:, None] * d.double()
        p64 = bc + ad
        binade = torch.floor(torch.log2(p64.abs().clamp_min(1e-300))).clamp_min(-14 if dtype == torch.float16 else -126)
        assert ((p.cpu().double() - p64).abs() <= ULP[dtype] * 2.0**binade + 2.0**-22 * (bc.abs() + ad.abs())).all()
        out2 = torch.empty_like(cd)
        _hip.launch_step(plan, [p if k == slot else t for k, t in enumerate(operands)], out2, None, seeds, numel, DEV)
        assert torch.equal(bits(out), bits(out2))
        assert torch.equal(bits(launch(only=True)[1]), bits(p))  # the guidance-only form: the same p
        if n % 2048 == 0:
            try:
                lib.skr_set_tuning(b"one_trip", 0)  # the grid-stride twin: the same bits
                out_gs, p_gs = launch()
            finally:
                lib.skr_set_tuning(b"one_trip", 1)
            assert torch.equal(bits(out_gs), bits(out)) and torch.equal(bits(p_gs), bits(p))


@pytest.mark.parametrize("sampler", [PT.DPM(order=2), PT.UniPC(order=2)], ids=["dpm2", "unipc2"])
def test_wrapper(sampler):
    "4 bf16 steps: prev_sample against a twin's step() over the stored prediction; the running average across steps and across runs"
    shape, beta, r, g = (3, 4, 32, 16), -0.5, 10.0, torch.Generator().manual_seed(2)
    w, twin = (PD.SkrampleWrapperScheduler(sampler, PS.Karras(PS.Scaled())) for _ in range(2))
    w.set_projected_guidance(eta=0.0, norm_threshold=r, momentum=beta)
    w.set_timesteps(4), twin.set_timesteps(4)
    x, m = (torch.randn(shape, generator=g) * float(w.init_noise_sigma)).bfloat16().to(DEV), torch.zeros(shape, dtype=torch.bfloat16)
    for t in w.timesteps:
        u, c = (torch.randn(shape, generator=g).bfloat16() for _ in range(2))
        d = restate_d(u, c, m, beta)
        assert (d.double().reshape(3, -1).pow(2).sum(1).sqrt() > 1.01 * r).all()  # the threshold clamps
        got = w.step_guided(u.to(DEV), c.to(DEV), G, t, x, return_dict=False)[0]
        ref = twin.step(w._raw_outputs[-1], t, x, return_dict=False)[0]
        assert torch.equal(bits(got), bits(ref)) and torch.equal(bits(w._projection.momentum_buf.cpu()), bits(d))
        x, m = got, d
    w.set_timesteps(4)
    assert not w._projection.momentum_buf.any()
