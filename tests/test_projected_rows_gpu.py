"""The row forms of adaptive projected guidance on the device.  Through the C ABI: skr_projected_guidance_coef_indexed[_per_sample] and
skr_projected_guided_step_launch_indexed[_per_sample] against the two direct entries run on every sample alone with its row's values, and
against the float64 bounds of test_projected_guidance_gpu.  Through capture_sampling_loop(projected=True): replays, retarget and per-sample
slots against the eager step_guided loop."""

import ctypes

import numpy as np
import pytest
import torch
from test_projected_guidance_gpu import bits
from test_projected_guidance_host import coefficients64, restate_d, restate_p
from test_thresholding_gpu import DEV, DTYPES, ULP, plan_for

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip, graphs
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
ids = lambda d: str(d).split(".")[1]  # noqa: E731
# (g, eta, r, beta, zeta0, stream0) of the three rows: plain guidance exactly; a clamp with negative momentum; positive momentum under a threshold above every norm
ROWS = [(7.5, 1.0, 0.0, 0.0, 0.3, 5), (5.0, 0.0, 10.0, -0.5, 0.2, 6), (3.0, 0.5, 1e6, 0.25, 0.1, 7)]
OFFSET = 2  # row_offset: the three rows stand behind two rows of zeros
PERM = [2, 0, 1]  # per-sample indices: sample s reads row PERM[s]


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("last", [False, True], ids=["slot0", "slot_last"])
@pytest.mark.parametrize("K", [2, 13])
@pytest.mark.parametrize("per_sample", [False, True], ids=["indexed", "per_sample"])
@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_c_abi(dtype, n, per_sample, K, last, noise):
    lib, slot, g = _hip.load(), (K - 1 if last else 0), torch.Generator().manual_seed(n + K)
    u, c, m = (torch.randn(3, n, generator=g).to(dtype) for _ in range(3))
    operands = [torch.randn(3, n, generator=g).to(dtype).to(DEV) for _ in range(K)]
    ud, cd = u.to(DEV), c.to(DEV)
    operands[slot] = ud
    seeds = torch.tensor([11, 12, 13], dtype=torch.int64, device=DEV) if noise else None
    coefs = [[0.9 - 0.17 * k + 0.05 * i for k in range(K)] for i in range(3)]
    plans = [plan_for(K, dtype, coefs[i], z if noise else 0.0, n) for i, (*_, z, _) in enumerate(ROWS)]
    table = [_hip.StepRowC() for _ in range(OFFSET)]
    for plan, (gs, eta, r, beta, _, stream) in zip(plans, ROWS):
        plan.stream0 = stream if noise else 0
        row = _hip.IndexedRows.row_from(plan)
        row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3] = gs, eta, r, beta
        table.append(row)
    rows_dev = torch.zeros(len(table) * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=DEV)
    _hip.upload_rows(rows_dev, 0, table)
    suffix = "_indexed_per_sample" if per_sample else "_indexed"
    arr = (ctypes.c_void_p * K)(*(t.data_ptr() for t in operands))
    for index in [PERM] if per_sample else [[i] * 3 for i in range(3)]:  # the row of every sample
        index_dev = torch.tensor(index if per_sample else index[:1], dtype=torch.int32, device=DEV)
        buf, coef = m.to(DEV), torch.full((6,), -7.0, dtype=torch.float32, device=DEV)
        partials = torch.empty(_hip.projected_partials(3 * n, n), dtype=torch.float64, device=DEV)
        out, p = torch.empty_like(cd), torch.empty_like(cd)
        where = (rows_dev.data_ptr(), index_dev.data_ptr(), OFFSET)
        status = getattr(lib, "skr_projected_guidance_coef" + suffix)(ud.data_ptr(), cd.data_ptr(), buf.data_ptr(), plans[0].dtype_a, 3 * n, n, *where, coef.data_ptr(), None,
                                                                      partials.data_ptr(), None)  # fmt: skip
        assert status == 0
        guide, proj = _hip.StepGuidanceC(cd.data_ptr(), p.data_ptr(), 0.0, slot, 0), _hip.StepProjectionC(coef.data_ptr(), buf.data_ptr(), n, 0)
        status = getattr(lib, "skr_projected_guided_step_launch" + suffix)(ctypes.byref(plans[0]), arr, out.data_ptr(), ctypes.byref(guide), ctypes.byref(proj),
                                                                           seeds.data_ptr() if noise else None, 3 * n, *where, None)  # fmt: skip
        assert status == 0
        for s, i in enumerate(index):  # sample s alone through the two direct entries, with the values of row i
            gs, eta, r, beta, *_ = ROWS[i]
            one = slice(s, s + 1)
            m1 = m[one].to(DEV) if beta != 0.0 else None
            coef1, part1 = torch.empty(2, dtype=torch.float32, device=DEV), torch.empty(_hip.projected_partials(n, n), dtype=torch.float64, device=DEV)
            _hip.launch_projected_coef(ud[one], cd[one], m1, gs, eta, r, beta, n, coef1, part1)
            out1, p1 = torch.empty_like(cd[one]), torch.empty_like(cd[one])
            _hip.launch_projected_guided_step(plans[i], [t[one] for t in operands], out1, cd[one], p1, slot, coef1, m1, n, seeds[one] if noise else None, n, DEV)
            assert torch.equal(bits(coef[2 * s : 2 * s + 2]), bits(coef1)) and torch.equal(bits(out[one]), bits(out1)) and torch.equal(bits(p[one]), bits(p1))
            assert torch.equal(bits(buf[one].cpu()), bits(m1.cpu() if beta != 0.0 else m[one]))  # a zero-momentum row leaves the sample's bytes alone
            # the float64 bounds of test_projected_guidance_gpu (test_statistic, test_step), as they stand
            d = restate_d(u[one], c[one], m[one], beta)
            assert torch.equal(bits(p1.cpu()), bits(restate_p(c[one], d, coef1[:1].cpu(), coef1[1:].cpu())))
            a_ref, b_ref, (_, _, scc, sadc) = coefficients64(d, c[one], gs, eta, r)
            a, b = coef1[:1].cpu().double(), coef1[1:].cpu().double()
            assert ((a - a_ref).abs() <= 2.0**-23 * a_ref.abs()).all(), (a, a_ref)
            assert ((b - b_ref).abs() <= 2.0**-23 * b_ref.abs() + 1e-9 * (a_ref * (1 - eta)).abs() * sadc / scc).all(), (b, b_ref)
            bc, ad = b_ref[:, None] * c[one].double(), a_ref[:, None] * d.double()
            p64 = bc + ad
            binade = torch.floor(torch.log2(p64.abs().clamp_min(1e-300))).clamp_min(-14 if dtype == torch.float16 else -126)
            assert ((p1.cpu().double() - p64).abs() <= ULP[dtype] * 2.0**binade + 2.0**-22 * (bc.abs() + ad.abs())).all()
            if i == 0:  # eta = 1, r = 0, beta = 0: plain guidance
                assert a == np.float32(gs - 1) and b == 1.0
            assert (a < np.float32(gs - 1)) == (i == 1)  # row 1 clamps, row 2's threshold lies above every norm


SETTINGS = [(dict(eta=0.0, norm_threshold=10.0, momentum=-0.5), 7.5), (dict(eta=0.5, norm_threshold=30.0, momentum=0.0), 4.0)]  # (projected setting, guidance scale)


def scheduler(setting):
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    w.set_projected_guidance(**setting)
    return w


@pytest.fixture(scope="module")
def loop_case():
    "(model, x0, the eager result of each setting): 4 bf16 DPM-2 steps on 3 x (4, 32, 16), the network two seeded affine maps of the sample"
    g = torch.Generator().manual_seed(4)
    wu, wc = (torch.randn(1, 4, 32, 16, generator=g).bfloat16().to(DEV) for _ in range(2))
    model = lambda x, t: (x * 0.5 + wu, x * 0.25 + wc)  # noqa: E731

    def eager(k, x):
        w = scheduler(SETTINGS[k][0])
        w.set_timesteps(4)
        for t in w.timesteps:
            x = w.step_guided(*model(x, t), SETTINGS[k][1], t, x, return_dict=False)[0]
        return x

    x0 = (torch.randn(3, 4, 32, 16, generator=g) * 14.6).bfloat16().to(DEV)
    return model, x0, eager


@pytest.mark.parametrize("mode", ["plain", "indexed", "per_sample"])
def test_captured_loop(loop_case, mode):
    model, x0, eager = loop_case
    options = dict(indexed=mode != "plain", per_sample=mode == "per_sample")
    loop = graphs.capture_sampling_loop(scheduler(SETTINGS[0][0]), model, x0, 4, guidance_scale=SETTINGS[0][1], projected=True, **options)
    first = loop(x0)
    assert torch.equal(bits(first), bits(eager(0, x0)))
    assert torch.equal(bits(loop(x0)), bits(first))  # the running average is cleared inside the graph
    if mode == "plain":
        return
    loop.retarget(scheduler(SETTINGS[1][0]), slot=1, guidance_scale=SETTINGS[1][1])  # another (eta, r, beta) and another scale: no re-capture
    assert torch.equal(bits(loop(x0, slot=1)), bits(eager(1, x0)))
    assert torch.equal(bits(loop(x0, slot=0)), bits(first))  # the dry run left the loop's own running average alone
    if mode == "per_sample":
        mixed = loop(x0, slot=[0, 1, 0])
        for s, k in enumerate([0, 1, 0]):  # every sample against its own setting's lone eager run
            assert torch.equal(bits(mixed[s : s + 1]), bits(eager(k, x0[s : s + 1])))
