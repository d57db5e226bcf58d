"""Rescaled guidance (guidance_rescale) on the device: the statistics launch, the rescaled step entry, the wrapper and captured loops.

What is compared, and against what:
  * the statistic's two standard deviations against the std computed exactly on the host (math.fsum over shifted float64 data) from
    the T-valued cond and p, relative tolerance 2^-30.  That figure is derived, not measured: the first-order worst-case bound of a
    length-n recursive double sum for  (S2 - S1^2 / n) / (n - 1)  is about 80 n 2^-53 while the pivot lies within 5 sigma of the mean
    (the test asserts that precondition on the host) -- 5.8e-10 at n = 65536, below 2^-30 = 9.3e-10; any fixed-order tree does better,
    and 2^-30 is still 64 times finer than an fp32 ulp;
  * the factor against the chain rn_T(rn_M(.)), division, rn_T recomputed on the host from the device's OWN two doubles, bit for bit
    (this tests the chain without depending on ties);
  * the step entry against torch's own device ops, live, fed with the factor tensor the statistics launch produced, and
    skr_step_launch with the result in `slot`: bit for bit, `out` and `guided_out`;
  * the wrapper against a twin wrapper stepping with step() over those torch lines: bit for bit.
Every comparison but the first is made on integer views of the bits."""

import itertools
import math

import pytest
import torch

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.graphs import capture_sampling_loop
from skrample_amd.sampling import lazy
from skrample_amd.sampling import structured as PT

pytestmark = pytest.mark.gpu

INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ALL_DTYPES = {**DTYPES, "fp64": torch.float64}
SCALES, PHIS = (7.5, 7.3), (0.7, 0.3, 1.0, 0.0)
STAT_TOLERANCE = 2.0**-30


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def same_bits(a, b):
    a, b = (v.materialize() if isinstance(v, lazy.LazyTensor) else v for v in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_VIEW[a.dtype]), b.contiguous().view(INT_VIEW[b.dtype]))


def differing(a, b):
    "how many elements differ in their bits, and the first few pairs: what a failing comparison prints"
    a, b = a.contiguous().view(INT_VIEW[a.dtype]).flatten(), b.contiguous().view(INT_VIEW[b.dtype]).flatten()
    at = (a != b).nonzero().flatten()
    return int(at.numel()), a.numel(), [(int(i), hex(int(a[i]) & 0xFFFFFFFF), hex(int(b[i]) & 0xFFFFFFFF)) for i in at[:4]]


def normal(shape, dtype, dev, seed, scale=1.0, mean=0.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + mean).to(dtype).to(dev)


def statistic(u, c, scale):
    "(factor [B], stats [B, 2]) of one statistics launch over contiguous device tensors of shape (B, ...)"
    batch = u.shape[0]
    factor = torch.zeros(batch, dtype=u.dtype, device=u.device)
    stats = torch.zeros(batch, 2, dtype=torch.float64, device=u.device)
    _hip.launch_guidance_factor(u, c, scale, u.numel() // batch, factor, stats)
    return factor, stats


# ---- 1. the statistic ----------------------------------------------------------------------------------------------------------------
def exact_std(values):
    "(unbiased std, |pivot - mean| / std) of a 1-D float64 tensor, exactly: math.fsum over the data shifted by its first element"
    n = values.numel()
    d = (values - values[0]).tolist()
    s1, s2 = math.fsum(d), math.fsum(v * v for v in d)
    std = math.sqrt(max((s2 - s1 * s1 / n) / (n - 1), 0.0))
    return std, abs(s1 / n) / std


def host_chain(std_c, std_p, dtype):
    "rn_T(div_M(rn_T(rn_M(std_c)), rn_T(rn_M(std_p)))) on the host"
    if dtype == torch.float64:
        return torch.tensor(std_c, dtype=torch.float64) / torch.tensor(std_p, dtype=torch.float64)
    a, b = (torch.tensor(v, dtype=torch.float64).to(torch.float32).to(dtype) for v in (std_c, std_p))
    return (a.to(torch.float32) / b.to(torch.float32)).to(dtype)


def check_statistic(u, c, scale):
    factor, stats = statistic(u, c, scale)
    p = u + scale * (c - u)  # (torch's own three device ops: the tensor it would take the std of)
    batch = u.shape[0]
    host_c, host_p, got = c.reshape(batch, -1).double().cpu(), p.reshape(batch, -1).double().cpu(), stats.cpu()
    for s in range(batch):
        for which, values in enumerate((host_c[s], host_p[s])):
            want, pivot_sigmas = exact_std(values)
            assert pivot_sigmas <= 5.0, (s, which, pivot_sigmas)  # the precondition of the derived bound
            error = abs(got[s, which].item() - want) / want
            print(f"std {tuple(u.shape)} {u.dtype} g={scale} sample {s} {'cp'[which]}: device {got[s, which].item():.17g} exact {want:.17g} rel {error:.3g}")
            assert error <= STAT_TOLERANCE, (tuple(u.shape), u.dtype, scale, s, which, got[s, which].item(), want, error)
        want_factor = host_chain(got[s, 0].item(), got[s, 1].item(), u.dtype)
        assert same_bits(factor[s].cpu().reshape(1), want_factor.reshape(1)), (tuple(u.shape), u.dtype, scale, s, factor[s].item(), want_factor.item())
    return factor, stats


STAT_SHAPES = [(3, 2048), (2, 4096), (2, 4, 10, 10), (2, 3, 10, 10), (1, 8), (2, 4, 128, 128)]


@pytest.mark.parametrize("shape", STAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(ALL_DTYPES))
def test_statistic_against_the_exact_std_and_the_factor_chain(name, shape, dev):
    "whole spans, several spans per sample, a ragged span, a second sample off a 16-byte boundary ((2, 3, 10, 10)), 8 elements, 32 spans"
    dtype = ALL_DTYPES[name]
    u, c = normal(shape, dtype, dev, 11), normal(shape, dtype, dev, 12)
    for scale in SCALES:
        check_statistic(u, c, scale)


def test_statistic_of_a_sample_whose_mean_is_far_above_its_std(dev):
    "fp32, mean 100 and std 0.01: unshifted sums would lose 2 log2(1e4) = 27 bits to cancellation; the pivot is what keeps the tolerance"
    shape = (2, 4, 128, 128)
    u, c = normal(shape, torch.float32, dev, 21, 0.01, 100.0), normal(shape, torch.float32, dev, 22, 0.01, 100.0)
    _, stats = check_statistic(u, c, 7.5)
    assert ((stats[:, 0] > 0.0099) & (stats[:, 0] < 0.0101)).all()


@pytest.mark.parametrize("sample", [(4, 128, 128), (4, 10, 10), (3, 10, 10)], ids=["32_spans", "ragged", "off_16_bytes"])
@pytest.mark.parametrize("name", sorted(ALL_DTYPES))
def test_a_sample_has_the_same_bits_alone_and_anywhere_in_a_batch_and_over_two_runs(name, sample, dev):
    """the partition depends on sample_numel and dtype only.  (fp16: the tail rule goes by the index in the whole launch, and these sizes
    keep a sample on one side of it alone and batched: 3 x 65536 has no tail, 3 x 400 and 3 x 300 lie below 2048 altogether)"""
    dtype = ALL_DTYPES[name]
    u1, c1 = normal((1, *sample), dtype, dev, 31), normal((1, *sample), dtype, dev, 32)
    others = [(normal((1, *sample), dtype, dev, 33 + 2 * k), normal((1, *sample), dtype, dev, 34 + 2 * k)) for k in range(2)]
    alone_f, alone_s = statistic(u1, c1, 7.3)
    again_f, again_s = statistic(u1, c1, 7.3)
    assert same_bits(alone_f, again_f) and same_bits(alone_s, again_s)
    for at in range(3):
        order = others[:at] + [(u1, c1)] + others[at:]
        f, s = statistic(torch.cat([o[0] for o in order]), torch.cat([o[1] for o in order]), 7.3)
        assert same_bits(f[at : at + 1], alone_f) and same_bits(s[at : at + 1], alone_s), (name, sample, at)


def test_statistic_for_the_record_against_torchs_own_device_std(dev):
    """not a gate: torch's device reduction order is not ours, so bit equality of the factor is not promised.  Prints (run with -s) how
    many samples of (8, 4, 32, 32) have the factor of the diffusers lines with torch's own std; tools/bench_guided_rescale.py records
    the same count in profiles/guided_rescale.txt."""
    for name in ("bf16", "fp32"):
        dtype = DTYPES[name]
        same = total = 0
        for seed in range(8):
            u, c = normal((8, 4, 32, 32), dtype, dev, 500 + 2 * seed), normal((8, 4, 32, 32), dtype, dev, 501 + 2 * seed)
            p = u + 7.5 * (c - u)
            theirs = c.std(dim=[1, 2, 3]) / p.std(dim=[1, 2, 3])
            ours, _ = statistic(u, c, 7.5)
            same += int((ours.view(INT_VIEW[dtype]) == theirs.view(INT_VIEW[dtype])).sum())
            total += 8
        print(f"factor against torch's device std, {name}: {same} of {total} samples have the same bits")
        assert total == 64


# ---- 2. the raw step entry -----------------------------------------------------------------------------------------------------------
def make_plan(n, dtype, draw, sample_numel, acc_f64=False):
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n
    plan.dtype_a = _hip.DTYPE_CODE[dtype]
    plan.dtype_b = _hip.DTYPE_CODE[torch.float64 if acc_f64 else torch.float32]
    plan.out0_dtype, plan.out1_dtype = _hip.DTYPE_CODE[dtype], _hip.NONE
    plan.acc_f64 = 1 if acc_f64 else 0
    for k in range(n):
        plan.coef0[k] = (-1.0) ** k * (0.3 + 0.17 * k)
    if draw:
        plan.noise_mode, plan.zeta0, plan.stream0, plan.sample_numel = 1, 0.45, 512, sample_numel
    return plan


def torch_lines(u, c, factor, scale, phi):
    "torch's own device ops with the factor tensor of the statistics launch"
    p = u + scale * (c - u)
    resc = p * factor.view(u.shape[0], *([1] * (u.ndim - 1)))
    return phi * resc + (1 - phi) * p


def check_case(dev, shape, dtype, n, slot, draw, store, scale, phi, seed, value_scale=1.0):
    inputs = [normal(shape, dtype, dev, seed + k, value_scale) for k in range(n)]
    cond = normal(shape, dtype, dev, seed + 100, value_scale)
    seeds = torch.tensor([11, 22, 33, 44][: shape[0]], dtype=torch.int64, device=dev)
    numel, sample_numel = inputs[0].numel(), inputs[0].numel() // shape[0]
    plan = make_plan(n, dtype, draw, sample_numel, acc_f64=dtype == torch.float64)
    uncond = inputs[slot]
    factor, _ = statistic(uncond, cond, scale)
    p_ref = torch_lines(uncond, cond, factor, scale, phi)
    assert p_ref.dtype == dtype
    want = torch.zeros(shape, dtype=dtype, device=dev)
    _hip.launch_step(plan, inputs[:slot] + [p_ref] + inputs[slot + 1 :], want, None, seeds if draw else None, numel, dev)
    got = torch.zeros(shape, dtype=dtype, device=dev)
    guided = torch.zeros_like(uncond) if store else None
    _hip.launch_step_guided_rescaled(plan, inputs, got, cond, guided, scale, slot, factor, phi, sample_numel, seeds if draw else None, numel, dev)
    what = (tuple(shape), str(dtype), n, slot, draw, store, scale, phi, value_scale)
    if store:
        assert same_bits(guided, p_ref), (what, differing(guided, p_ref))
    assert same_bits(got, want), (what, differing(got, want))
    return got, guided


def check_guidance_only(dev, shape, dtype, scale, phi, seed, value_scale=1.0):
    u, c = normal(shape, dtype, dev, seed, value_scale), normal(shape, dtype, dev, seed + 1, value_scale)
    factor, _ = statistic(u, c, scale)
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 1
    plan.dtype_a = plan.dtype_b = _hip.DTYPE_CODE[dtype]
    plan.out0_dtype = plan.out1_dtype = _hip.NONE
    plan.acc_f64 = 1 if dtype == torch.float64 else 0
    plan.coef0[0] = 1.0
    p = torch.zeros_like(u)
    _hip.launch_step_guided_rescaled(plan, [u], None, c, p, scale, 0, factor, phi, u.numel() // shape[0], None, u.numel(), dev)
    want = torch_lines(u, c, factor, scale, phi)
    assert same_bits(p, want), (tuple(shape), str(dtype), scale, phi, value_scale, differing(p, want))


def slots_of(n):
    return sorted({0, n // 2, n - 1})


# (shape, the draws it runs with): the one-trip kernel's -- one chunk per sample, and two chunks per sample in three samples -- and the
# general kernel's: ragged with samples of a multiple of 8 (draws), ragged with the second sample off a 16-byte boundary, 8 elements
GRID_SHAPES = {
    "one_trip": ((2, 2048), (False, True)),
    "one_trip_3x2": ((3, 4096), (False, True)),
    "ragged_draw": ((2, 4, 10, 10), (True,)),
    "ragged": ((2, 3, 10, 10), (False,)),
    "eight": ((1, 8), (False, True)),
}
MIXES = list(itertools.product(PHIS, SCALES))  # every phi with every scale, rotating through the cases


@pytest.mark.parametrize("kind", sorted(GRID_SHAPES))
@pytest.mark.parametrize("n", (1, 4, 5, 16))
@pytest.mark.parametrize("name", sorted(DTYPES))
def test_raw_entry_equals_torch_plus_step_launch(name, n, kind, dev):
    """dtype x operand count x slot first / middle / last x with and without a draw x with and without guided_out, every phi with every
    scale rotating through the cases, and the guidance-only form on the same shape.
    fp16 on the three general-kernel shapes settles the tail rule of the two scalar products: every element of these tensors lies in
    the partial last block of torch's tensor-times-number kernel, where it rounds the product once."""
    dtype = DTYPES[name]
    shape, draws = GRID_SHAPES[kind]
    mixes = itertools.cycle(MIXES[n % len(MIXES) :] + MIXES[: n % len(MIXES)])
    for slot, draw, store in itertools.product(slots_of(n), draws, (False, True)):
        phi, scale = next(mixes)
        check_case(dev, shape, dtype, n, slot, draw, store, scale, phi, seed=1000 * n + slot)
    phi, scale = next(mixes)
    check_guidance_only(dev, shape, dtype, scale, phi, seed=3000 + n)


@pytest.mark.parametrize("kind", sorted(GRID_SHAPES))
@pytest.mark.parametrize("name,value_scale", [("bf16", 1.0), ("fp16", 1.0), ("fp16", 1e-4), ("fp32", 1.0), ("fp64", 1.0)])
def test_every_phi_with_every_scale_on_every_value_set(name, value_scale, kind, dev):
    "all eight (phi, scale) pairs per dtype and shape, the fp16 set scaled by 1e-4 (subnormal results) and fp64 (the general kernel) among them"
    dtype = ALL_DTYPES[name]
    shape, draws = GRID_SHAPES[kind]
    for k, (phi, scale) in enumerate(MIXES):
        _, guided = check_case(dev, shape, dtype, 3, 1, draws[-1] and k % 2 == 0, True, scale, phi, seed=7 + k, value_scale=value_scale)
        if value_scale == 1e-4 and guided.numel() >= 600:
            assert (guided.float().abs() < 2.0**-14).any()  # subnormal results
        check_guidance_only(dev, shape, dtype, scale, phi, seed=40 + k, value_scale=value_scale)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_the_two_kernels_agree_bit_for_bit(name, dev):
    "the one-trip shapes again with one_trip 0: the general kernel gives the one-trip kernel's bits (and torch's)"
    lib, dtype = _hip.load(), DTYPES[name]
    for shape, n, draw in itertools.product(((2, 2048), (3, 4096)), (1, 4, 5, 16), (False, True)):
        a, pa = check_case(dev, shape, dtype, n, n // 2, draw, True, 7.3, 0.7, seed=50 * n)
        assert lib.skr_set_tuning(b"one_trip", 0) == 0
        try:
            b, pb = check_case(dev, shape, dtype, n, n // 2, draw, True, 7.3, 0.7, seed=50 * n)
        finally:
            lib.skr_set_tuning(b"one_trip", 1)
        assert same_bits(a, b) and same_bits(pa, pb), (shape, n, draw)


def test_a_drawing_plan_with_another_sample_is_refused_on_the_device_too(dev):
    u, c = normal((2, 4096), torch.bfloat16, dev, 1), normal((2, 4096), torch.bfloat16, dev, 2)
    factor, _ = statistic(u, c, 7.5)
    out = torch.zeros_like(u)
    seeds = torch.tensor([1, 2], dtype=torch.int64, device=dev)
    with pytest.raises(_hip.SkrampleHipError, match="skr_step_launch_guided_rescaled"):
        _hip.launch_step_guided_rescaled(make_plan(1, torch.bfloat16, True, 2048), [u], out, c, None, 7.5, 0, factor, 0.7, 4096, seeds, u.numel(), dev)
    torch.cuda.synchronize()
    assert not out.any()


# ---- 3. the wrapper ------------------------------------------------------------------------------------------------------------------
LATENTS, STEPS, SCALE, PHI = (2, 4, 32, 32), 4, 7.3, 0.7
ONE_LAUNCH = {
    "euler": lambda: PT.Euler(),
    "dpm2": lambda: PT.DPM(order=2),
    "dpm2_sde": lambda: PT.DPM(order=2, stochasticity=1),
    "adams3": lambda: PT.Adams(order=3),
    "unip2": lambda: PT.UniP(order=2),
}
TWO_LAUNCH = {"unipc2": lambda: PT.UniPC(order=2), "spc": lambda: PT.SPC()}


def lines(u, c, scale, phi):
    "the pipeline's lines with the factor of Guidance.factor() where torch would take its own two stds"
    p = u + scale * (c - u)
    if phi == 0.0:
        return p
    return phi * (p * lazy.Guidance(u, c, scale).factor()) + (1 - phi) * p


def network_outputs(dev, dtype, seed, channels_last=False):
    g = torch.Generator().manual_seed(seed)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    x = torch.randn(LATENTS, generator=g).to(dtype).to(dev).contiguous(memory_format=fmt)
    outs = [tuple(h.contiguous(memory_format=fmt) for h in torch.randn((2 * LATENTS[0], *LATENTS[1:]), generator=g).to(dtype).to(dev).chunk(2)) for _ in range(STEPS)]
    return x, outs


def twins(sampler, dev, launches, phi_at=lambda i: PHI, prepare=lambda w: None, channels_last=False, **fields):
    """twin wrappers: one stepping with step_guided(..., guidance_rescale=phi), the other with step() over the torch lines;
    prev_sample and pred_original_sample equal in every bit at every step.  `launches`: the trace of a rescaled step -- the statistic
    first, then that many step launches, the first of them the rescaled one; phi_at(i) None: a plain step() of the lines without rescale"""
    make = lambda: PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled()), **fields)  # noqa: E731
    fused, plain = make(), make()
    fused.set_timesteps(STEPS), plain.set_timesteps(STEPS)
    prepare(fused), prepare(plain)
    x, outs = network_outputs(dev, torch.bfloat16, 77, channels_last)
    gens = [[torch.Generator().manual_seed(s) for s in (1234, 5678)] for _ in range(2)]
    xa = xb = x
    for i, t in enumerate(plain.timesteps.tolist()):
        uncond, cond = outs[i]
        phi = phi_at(i)
        if phi is None:
            xa, pa = fused.step(lines(uncond, cond, SCALE, 0.0), t, xa, generator=gens[0], return_dict=False)
        else:
            _hip.trace = []
            try:
                xa, pa = fused.step_guided(uncond, cond, SCALE, t, xa, generator=gens[0], return_dict=False, guidance_rescale=phi)
                trace = list(_hip.trace)
            finally:
                _hip.trace = None
            if launches is not None and phi != 0.0:
                assert [e.kind == "guidance_factor" for e in trace] == [True] + [False] * launches and trace[1].kind == "guided_rescaled", (i, [e.kind for e in trace])
            elif launches is not None:
                assert len(trace) == launches and all(e.kind not in ("guided_rescaled", "guidance_factor") for e in trace), (i, [e.kind for e in trace])
        xb, pb = plain.step(lines(uncond, cond, SCALE, phi or 0.0), t, xb, generator=gens[1], return_dict=False)
        assert xa.dtype == torch.bfloat16 and same_bits(xa, xb) and xa.stride() == xb.stride(), i
        assert same_bits(pa, pb), i
    return fused


@pytest.mark.parametrize("name", sorted(ONE_LAUNCH))
def test_wrapper_rescaled_step_is_the_statistic_and_one_launch(name, dev):
    fused = twins(ONE_LAUNCH[name], dev, 1)
    assert not fused._programs and not fused._fast  # no step program, no replayed entry


@pytest.mark.parametrize("name", sorted(TWO_LAUNCH))
def test_wrapper_two_output_samplers_take_the_guidance_only_form(name, dev):
    twins(TWO_LAUNCH[name], dev, 2)


def test_wrapper_under_set_inpaint_and_compute_scale_none_and_channels_last(dev):
    "what the one launch does not cover: the statistic, the rescaled guidance-only launch, then the step as ever"
    g = torch.Generator().manual_seed(5)
    orig, nz = (torch.randn(LATENTS, generator=g).bfloat16().to(dev) for _ in range(2))
    mask = (torch.rand((2, 1, 32, 32), generator=g) < 0.5).to(dev)
    twins(ONE_LAUNCH["dpm2"], dev, 2, prepare=lambda w: w.set_inpaint(mask, orig, nz))
    twins(ONE_LAUNCH["dpm2"], dev, None, compute_scale=None)  # (the op tape's launch is not a step launch: not counted)
    twins(ONE_LAUNCH["dpm2"], dev, 2, channels_last=True)


@pytest.mark.parametrize("name", ["dpm2", "adams3", "unipc2"])
def test_wrapper_run_that_mixes_rescaled_guided_and_plain_steps(name, dev):
    "calls with rescale, with guidance_rescale=0.0 (today's launches, today's trace tuples) and plain step() calls in one run"
    mix = {0: PHI, 1: 0.0, 2: None, 3: 0.3}
    twins({**ONE_LAUNCH, **TWO_LAUNCH}[name], dev, 2 if name in TWO_LAUNCH else 1, phi_at=lambda i: mix[i])


def test_guidance_rescale_zero_is_the_call_without_the_keyword(dev):
    make = lambda: PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))  # noqa: E731
    x, outs = network_outputs(dev, torch.bfloat16, 81)
    results = []
    for kw in (dict(guidance_rescale=0.0), {}):
        w = make()
        w.set_timesteps(STEPS)
        _hip.trace = []
        try:
            out = w.step_guided(outs[0][0], outs[0][1], SCALE, w.timesteps.tolist()[0], x, return_dict=False, **kw)
            results.append((out, [(e.kind, e[5], e.scale, e.slot) for e in _hip.trace]))
        finally:
            _hip.trace = None
    (ra, ta), (rb, tb) = results
    assert ta == tb and len(ta) == 1 and ta[0][0] == "guided"  # one launch_step_guided record
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


def net(x, t):  # elementwise, two outputs (uncond, cond), ignores t
    return x * 0.5 + 0.3 * x.abs(), x * 0.25 - 0.1 * x.abs()


@pytest.mark.parametrize("name", ["dpm2_sde", "unipc2"])
def test_captured_loop_with_guidance_rescale_replays_the_eager_run(name, dev):
    "indexed=False: the statistics launch and the rescaled step are captured, phi frozen"
    sampler = {**ONE_LAUNCH, **TWO_LAUNCH}[name]
    seeds = [31, 32]
    x0 = torch.randn(LATENTS, generator=torch.Generator().manual_seed(41)).bfloat16().to(dev)
    w = PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled()))
    w.set_timesteps(STEPS)
    x = x0
    for t in w.timesteps.tolist():
        uncond, cond = net(x, t)
        x = w.step_guided(uncond, cond, SCALE, t, x, generator=list(seeds), return_dict=False, guidance_rescale=PHI)[0]
    eager = x.clone()
    loop = capture_sampling_loop(PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled())), net, x0, STEPS, seeds=seeds, guidance_scale=SCALE, guidance_rescale=PHI)
    assert loop.rows is None
    assert same_bits(loop(x0).clone(), eager) and same_bits(loop(x0).clone(), eager)
    plain = capture_sampling_loop(PD.SkrampleWrapperScheduler(sampler(), PS.Karras(PS.Scaled())), net, x0, STEPS, seeds=seeds, guidance_scale=SCALE)
    assert not same_bits(plain(x0).clone(), eager)  # (the rescale is not a no-op on these inputs)


@pytest.mark.parametrize("per_sample", [False, True])
def test_indexed_capture_with_guidance_rescale_is_refused_before_a_stream_captures(per_sample, dev):
    x0 = torch.randn(LATENTS, generator=torch.Generator().manual_seed(41)).bfloat16().to(dev)
    w = PD.SkrampleWrapperScheduler(PT.DPM(order=2), PS.Karras(PS.Scaled()))
    with pytest.raises(_hip.SkrampleHipError, match="guidance_rescale.*no row form") as caught:
        capture_sampling_loop(w, net, x0, STEPS, seeds=[31, 32], indexed=True, per_sample=per_sample, guidance_scale=SCALE, guidance_rescale=PHI)
    del caught  # (a caught exception kept in its own frame is a reference cycle)
    assert not torch.cuda.is_current_stream_capturing() and _hip.indexed is None
