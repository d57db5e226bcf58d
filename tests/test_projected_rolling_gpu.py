"""Projected guidance in rolling batches (needs an MI355X): skr_projected_guidance_coef_rolling and skr_projected_guided_step_launch_rolling
through the C ABI, inside an arena, against the two direct entries on each slot alone and against the float64 bounds of
test_projected_guidance_gpu; `RollingBatch(..., guided=True, projected=True)` against every request's lone eager step_guided run."""

import ctypes
import functools
import math

import pytest
import torch
from arena import Arena, untouched
from test_projected_guidance_gpu import bits, ids
from test_projected_guidance_host import DTYPE, NULL, UNSUPPORTED, coefficients64, restate_d
from test_thresholding_gpu import DEV, DTYPES, ULP, plan_for

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.rolling import RollingBatch
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu
# (g, eta, r, beta, stream1) of a row: zero momentum (plain guidance exactly); a running average that continues; one that starts, under either sign
ROWS = {"zero": (7.5, 1.0, 0.0, 0.0, 0), "cont": (5.0, 0.0, 10.0, -0.5, 0), "start-": (5.0, 0.0, 10.0, -0.5, 1), "start+": (3.0, 0.5, 1e6, 0.5, 1)}
PAIRS = [("zero", "cont"), ("start+", "start-")]  # the rows of slot 2 and slot 0; slot 1 is inactive
INDEX, OFFSET = [1, -1, 0], 1  # (a negative entry is tested before row_offset is added: -1 + 1 would be a row)


def launched(dtype, n, pair, K=2, last=False, noise=False):
    """both rolling launches inside an arena, whose poison is a NaN pattern in every dtype: the momentum slices of the inactive slot, of a
    zero-momentum slot and of a STARTING slot hold it; slot 2's row lacks one non-slot operand, whose slice there is NaN.  Returns what the
    launches left, and per active slot what the two direct entries give that sample alone (a starting row's from a zeroed buffer)."""
    g, arena, slot, kind = torch.Generator().manual_seed(n + K), Arena(DEV), (K - 1 if last else 0), {0: pair[1], 2: pair[0]}
    take = lambda name, count=3 * n, dt=dtype: arena.take(name, count, dt)  # noqa: E731
    operands, (cond, mom, out, p) = [take(f"in{j}").view(3, n) for j in range(K)], (take(name).view(3, n) for name in ("cond", "mom", "out", "p"))
    for t in (*operands, cond):
        t.copy_(torch.randn(3, n, generator=g).to(dtype))
    operands[slot][:, :4], cond[:, :4] = 0.0, -0.0  # c - u = -0: a starting row with positive beta stores +0
    for b, name in kind.items():
        if name == "cont":
            mom[b].copy_((torch.randn(n, generator=g) * 0.5).to(dtype))
    before, absent = mom.clone(), (slot + 1) % K
    coefs = [[0.9 - 0.17 * k + 0.05 * i for k in range(K)] for i in range(2)]
    coefs[0][absent] = 0.0
    operands[absent][2].fill_(math.nan)
    table = [_hip.StepRowC()]
    for i, name in enumerate(pair):
        plan = plan_for(K, dtype, coefs[i], 0.3 if noise else 0.0, n)
        plan.stream0 = 6 + i
        row = _hip.IndexedRows.row_from(plan)
        row.convert_k[0], row.convert_k[1], row.convert_k[2], row.convert_k[3], row.stream1 = ROWS[name]
        table.append(row)
    rows_dev = torch.zeros(len(table) * ctypes.sizeof(_hip.StepRowC), dtype=torch.uint8, device=DEV)
    _hip.upload_rows(rows_dev, 0, table)
    index, seeds = torch.tensor(INDEX, dtype=torch.int32, device=DEV), torch.tensor([11, 12, 13], dtype=torch.int64, device=DEV) if noise else None
    coef, stats, partials = take("coef", 6, torch.float32), take("stats", 9, torch.float64), take("partials", _hip.projected_partials(3 * n, n), torch.float64)
    lib, where, code = _hip.load(), (rows_dev.data_ptr(), index.data_ptr(), OFFSET), _hip.DTYPE_CODE[dtype]
    assert lib.skr_projected_guidance_coef_rolling(operands[slot].data_ptr(), cond.data_ptr(), mom.data_ptr(), code, 3 * n, n, *where, coef.data_ptr(), stats.data_ptr(),
                                                   partials.data_ptr(), None) == 0  # fmt: skip
    guide, proj = _hip.StepGuidanceC(cond.data_ptr(), p.data_ptr(), 0.0, slot, 0), _hip.StepProjectionC(coef.data_ptr(), mom.data_ptr(), n, 0)
    wide = plan_for(K, dtype, [0.0] * K, 1.0 if noise else 0.0, n)  # (the plan's scalars are not the rows')
    assert lib.skr_projected_guided_step_launch_rolling(ctypes.byref(wide), _hip._operand_array(operands), out.data_ptr(), ctypes.byref(guide), ctypes.byref(proj),
                                                        _hip._ptr(seeds), 3 * n, *where, None) == 0  # fmt: skip
    torch.cuda.synchronize()
    arena.check()
    got, want = dict(coef=coef.view(3, 2), stats=stats.view(3, 3), mom=mom, out=out, p=p), {}
    for b, name in kind.items():
        (gs, eta, r, beta, _), one, i = ROWS[name], slice(b, b + 1), pair.index(name)
        m0 = None if beta == 0.0 else before[one].clone() if name == "cont" else torch.zeros_like(before[one])
        m1 = None if m0 is None else m0.clone()
        coef1, stats1, part1 = torch.empty(2, dtype=torch.float32, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV), torch.empty_like(partials)
        _hip.launch_projected_coef(operands[slot][one], cond[one], m1, gs, eta, r, beta, n, coef1, part1, stats1)
        present = [j for j in range(K) if j == slot or coefs[i][j] != 0.0]
        lone = plan_for(len(present), dtype, [coefs[i][j] for j in present], 0.3 if noise else 0.0, n)
        lone.stream0 = 6 + i
        out1, p1 = torch.empty_like(cond[one]), torch.empty_like(cond[one])
        _hip.launch_projected_guided_step(lone, [operands[j][one] for j in present], out1, cond[one], p1, present.index(slot), coef1, m1, n, seeds[one] if noise else None, n, DEV)
        want[b] = dict(coef=coef1, stats=stats1, mom=m1, out=out1[0], p=p1[0], m0=m0, row=ROWS[name], u=operands[slot][one].cpu(), c=cond[one].cpu())
    return got, want


@pytest.mark.parametrize("pair", PAIRS, ids="/".join)
@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("last", [False, True], ids=["slot0", "slot_last"])
@pytest.mark.parametrize("K", [2, 6, 13])
@pytest.mark.parametrize("n", [2048, 4096])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_c_abi(dtype, n, K, last, noise, pair):
    got, want = launched(dtype, n, pair, K, last, noise)
    assert all(untouched(t[1]) for t in got.values())  # the inactive slot: coef, stats, momentum, out and p keep every byte
    for b, w in want.items():
        assert torch.equal(bits(got["coef"][b]), bits(w["coef"])) and torch.equal(bits(got["stats"][b]), bits(w["stats"])), b
        assert untouched(got["mom"][b]) if w["mom"] is None else torch.equal(bits(got["mom"][b]), bits(w["mom"][0])), b
        assert torch.isfinite(w["out"].float()).all()  # the absent operand's NaN reached neither run
        assert torch.equal(bits(got["out"][b]), bits(w["out"])) and torch.equal(bits(got["p"][b]), bits(w["p"])), b
        if dtype == torch.bfloat16 and n == 4096 and K == 6 and not last and not noise:  # the float64 bounds of test_projected_guidance_gpu's test_statistic and test_step, as they stand
            (gs, eta, r, beta, _), u, c = w["row"], w["u"], w["c"]
            d = restate_d(u, c, w["m0"].cpu() if beta != 0.0 else u, beta)
            assert beta == 0.0 or torch.equal(bits(got["mom"][b : b + 1].cpu()), bits(d))
            a_ref, b_ref, (sdd, sdc, scc, sadc) = coefficients64(d, c, gs, eta, r)
            sums = got["stats"][b : b + 1].cpu()
            for k, (ref, terms) in enumerate(((sdd, sdd), (sdc, sadc), (scc, scc))):
                assert ((sums[:, k] - ref).abs() <= n * 2.0**-52 * terms).all(), (k, sums[:, k], ref)
            a, bb = got["coef"][b, :1].cpu().double(), got["coef"][b, 1:].cpu().double()
            assert ((a - a_ref).abs() <= 2.0**-23 * a_ref.abs()).all(), (a, a_ref)
            assert ((bb - b_ref).abs() <= 2.0**-23 * b_ref.abs() + 1e-9 * (a_ref * (1 - eta)).abs() * sadc / scc).all(), (bb, b_ref)
            bc, ad = b_ref[:, None] * c.double(), a_ref[:, None] * d.double()
            binade = torch.floor(torch.log2((bc + ad).abs().clamp_min(1e-300))).clamp_min(-126)
            assert ((got["p"][b : b + 1].cpu().double() - (bc + ad)).abs() <= ULP[dtype] * 2.0**binade + 2.0**-22 * (bc.abs() + ad.abs())).all()


@pytest.mark.parametrize("changes,codes", [({"index": None}, (NULL, NULL)), ({"row_offset": -1}, (UNSUPPORTED, UNSUPPORTED)), ({"sn": 2056}, (UNSUPPORTED, UNSUPPORTED)),
                                           ({"dtype": _hip.F64}, (UNSUPPORTED, DTYPE))], ids=lambda v: str(v))  # fmt: skip
def test_argument_checks(changes, codes):
    "(statistic, step): no launch is reached"
    a = {"index": 1, "row_offset": 0, "sn": 2048, "dtype": _hip.BF16, **changes}
    buf = torch.zeros(3 * 4096, dtype=torch.float64, device=DEV)
    ptr, index, numel = buf.data_ptr(), (buf.data_ptr() if a["index"] else None), 3 * a["sn"]
    lib, plan = _hip.load(), plan_for(2, torch.bfloat16, [1.0, 1.0])
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = a["dtype"]
    assert lib.skr_projected_guidance_coef_rolling(ptr, ptr, ptr, a["dtype"], numel, a["sn"], ptr, index, a["row_offset"], ptr, None, ptr, None) == codes[0]
    guide, proj = _hip.StepGuidanceC(ptr, ptr, 0.0, 0, 0), _hip.StepProjectionC(ptr, ptr, a["sn"], 0)
    assert lib.skr_projected_guided_step_launch_rolling(ctypes.byref(plan), (ctypes.c_void_p * 2)(ptr, ptr), ptr, ctypes.byref(guide), ctypes.byref(proj), None, numel, ptr,
                                                        index, a["row_offset"], None) == codes[1]  # fmt: skip


# ---- rolling batches ---------------------------------------------------------------------------------------------------------------------
UNIT, CAPACITY = (4, 32, 16), 3
SAMPLERS = {"dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1.0), "euler": PT.Euler}
SCHEDULES = [lambda: PS.Karras(PS.Scaled()), lambda: PS.Scaled(), lambda: PS.Exponential(PS.Scaled())]
# (tick of admission, slot, steps, schedule, seed, (eta, norm_threshold, momentum), guidance scale or schedule): the fourth, with momentum, goes
# into the slot the first -- a momentum request too -- has left
REQUESTS = [(0, 0, 5, 0, 11, (0.0, 10.0, -0.5), 7.5), (1, 2, 3, 1, 12, (0.5, 30.0, 0.0), 4.0), (2, 1, 4, 2, 13, (1.0, 0.0, 0.5), [3.0, 4.0, 5.0, 6.0]),
            (5, 0, 3, 0, 14, (0.0, 10.0, -0.75), 5.0)]  # fmt: skip


def wrapper_of(name, which=0, setting=(0.0, 10.0, -0.5)):
    w = PD.SkrampleWrapperScheduler(SAMPLERS[name](), SCHEDULES[which]())
    w.set_projected_guidance(*setting)
    return w


@functools.lru_cache(maxsize=None)
def yardstick(name):
    "(model, latents, lone eager results) of the four requests: computed once per sampler and shared, never written to"
    g = torch.Generator().manual_seed(4)
    wu, wc = (torch.randn(1, *UNIT, generator=g).bfloat16().to(DEV) for _ in range(2))
    model = lambda x, t: (x * 0.5 + wu, x * 0.25 + wc)  # noqa: E731
    latents = [(torch.randn(UNIT, generator=g) * float(wrapper_of(name).init_noise_sigma)).bfloat16().to(DEV) for _ in REQUESTS]
    refs = []
    for (_, _, steps, which, seed, setting, scale), x in zip(REQUESTS, latents):
        w, x = wrapper_of(name, which, setting), x.unsqueeze(0)
        w.set_timesteps(steps)
        for i, t in enumerate(w.timesteps.tolist()):
            x = w.step_guided(*model(x, t), scale[i] if isinstance(scale, list) else scale, t, x, generator=[seed], return_dict=False)[0]
        refs.append(x[0].clone())
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.float()).all() for r in refs)
    return model, latents, refs


@pytest.mark.parametrize("name,mode", [("dpm2_sde", "host"), ("euler", "host"), ("dpm2_sde", "device"), ("dpm2_sde", "captured")], ids=lambda v: str(v))
def test_every_request_equals_its_lone_eager_run(name, mode):
    model, latents, refs = yardstick(name)
    example = torch.zeros((CAPACITY, *UNIT), dtype=torch.bfloat16, device=DEV)
    batch = RollingBatch(lambda: wrapper_of(name), example, capacity=CAPACITY, max_steps=8, guided=True, projected=True, device_positions=mode != "host")
    for t in (*batch.ring_tensors(), batch.momentum_buf):  # what a previous occupant may have left: nothing is zeroed per admission
        t.fill_(math.nan)
    ticks = batch.capture(model) if mode == "captured" else None

    def tick():
        if mode == "device":
            batch.advance()
        return ticks.tick() if ticks is not None else batch.step_guided(*model(batch.latents, batch.timesteps))

    results, resident, now = {}, {}, 0
    while len(results) < len(REQUESTS):
        for k, (at, slot, steps, which, seed, setting, scale) in enumerate(REQUESTS):
            if at == now:
                batch.admit(slot, latents[k], wrapper_of(name, which, setting), steps, seed=seed if name == "dpm2_sde" else None, guidance_scale=scale)
                resident[slot] = k
        for slot in tick():
            results[resident.pop(slot)] = batch.take(slot)
        now += 1
    torch.cuda.synchronize()
    for k, ref in enumerate(refs):
        assert torch.equal(bits(results[k]), bits(ref)), (name, mode, k, int((bits(results[k]) != bits(ref)).sum()))
