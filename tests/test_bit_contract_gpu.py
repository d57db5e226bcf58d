"""Every step-family launch against the exact model of its fp32 arithmetic (tests/bit_model.py), bit for bit over all elements: no
tolerance, no share of elements left out.  The inputs (tests/bit_cases.py) are the ones at which a kernel that fuses the last fma with
the conversion, splits an fma, changes the order, flushes subnormals, loses the sign of a zero or mishandles inf / NaN in one store path
gives other bits; tests/test_bit_model_host.py counts, on the host, how many elements each such kernel would miss.

  launch                                  kernels reached
  skr_step_launch, one output             step_kernel_k1 (whole chunks); step_kernel_k / step_kernel ("one_trip" 0, and three elements
                                          more than whole chunks: the scalar tail); fp32 with and without the tile layout ("tile")
  same, mixed groups                      step_kernel: 16-bit + fp32 operands, 16-bit and fp32 outputs
  skr_step_launch, two outputs            step_kernel_k2 ("two_out" 2) and step_kernel ("two_out" 0, ragged), fp32 out0 + 16-bit out1
  skr_step_launch_masked                  masked_kernel_v1; masked_kernel_gen ("one_trip" 0, ragged samples, fp32 operands under a 16-bit mask)
  skr_step_backward_launch                step_bwd_k1, step_bwd_general; one and two incoming gradients
  skr_step_masked_backward_launch         masked_bwd_k1, masked_bwd_general
  skr_step_launch, rounded conversion     step_kernel_rk1 (128 and 256 threads, K = 2, 4, 5, 8, the noisy last stage), step_kernel_rk (1, 2, 4
  (Runge-Kutta stages)                    vectors per lane, tile and no tile), step_kernel<..., CONV> (ragged body and scalar tail, more than 8
                                          operands, mixed dtypes, noise, acc_f64 out0): the routing table in front of the stage tests below.
                                          The table forms of step_kernel_rk1 stand on these through tests/test_table_forms_gpu.py, which holds
                                          every table instantiation bit for bit to the narrow launch.

In-kernel noise.  The Philox normals are not reproducible on the host to the bit (the oracle bar is table_cases.NORMAL_BAR), so they
are an INPUT of the model: an fp32-output launch of the same geometry, seeds and stream over one operand of zeros with coefficient 0
and zeta0 = 1 returns exactly z.  The extraction is anchored (the one-trip, the grid-stride and the no-tile kernel return the same bits,
within the bar of the oracle's normals), then every noisy launch must have the bits of the model fed with that z."""

import contextlib
from dataclasses import dataclass

import bit_cases as BC
import bit_model as BM
import numpy as np
import pytest
import table_cases as TC
import torch
from skr_oracle import noise as ON

from skrample_amd import _hip
from skrample_amd.sampling import lazy

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CODE = _hip.DTYPE_CODE
ROWS = BC.SAMPLES * BC.SAMPLE


@contextlib.contextmanager
def tuning(**switches):
    lib = _hip.load()
    try:
        for key, value in switches.items():
            assert lib.skr_set_tuning(key.encode(), value) == 0, key
        yield
    finally:
        lib.skr_set_tuning(b"reset", 0)


def on_device(ts):
    return [t.to(DEV) for t in ts]


def launch(ops, coef0, out0=None, coef1=None, chain=0.0, out1=None, zeta0=0.0, stream0=0, zeta1=0.0, stream1=0, seeds=None, sample=None):
    "one skr_step_launch over host operands (a leading group of one dtype, then at most one other); returns the outputs on the host"
    n, da = len(ops), ops[0].dtype
    na = next((j for j, t in enumerate(ops) if t.dtype != da), n)
    assert all(t.dtype == ops[-1].dtype for t in ops[na:])
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a = n, na, CODE[da]
    plan.dtype_b = CODE[ops[-1].dtype] if na < n else _hip.F32
    plan.out0_dtype = CODE[out0] if out0 is not None else _hip.NONE
    plan.out1_dtype = CODE[out1] if out1 is not None else _hip.NONE
    for k in range(n):
        plan.coef0[k] = coef0[k]
        plan.coef1[k] = coef1[k] if coef1 is not None else 0.0
    plan.chain, plan.zeta0, plan.zeta1, plan.stream0, plan.stream1 = chain, zeta0, zeta1, stream0, stream1
    numel = ops[0].numel()
    plan.noise_mode = 1 if (zeta0 != 0.0 or zeta1 != 0.0) else 0
    plan.sample_numel = sample if sample is not None else numel
    o0 = torch.empty(numel, dtype=out0, device=DEV) if out0 is not None else None
    o1 = torch.empty(numel, dtype=out1, device=DEV) if out1 is not None else None
    _hip.launch_step(plan, on_device(ops), o0, o1, seeds.to(DEV) if seeds is not None else None, numel, DEV)
    torch.cuda.synchronize()
    return tuple(o.cpu() for o in (o0, o1) if o is not None)


def launch_masked(ops, coef0, coef1, mask, mask_numel, batch_stride, out, sample, zeta0=0.0, stream0=0, seeds=None):
    n, da = len(ops), ops[0].dtype
    na = next((j for j, t in enumerate(ops) if t.dtype != da), n)
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a = n, na, CODE[da]
    plan.dtype_b = CODE[ops[-1].dtype] if na < n else _hip.F32
    plan.out0_dtype, plan.out1_dtype = CODE[out], _hip.NONE
    for k in range(n):
        plan.coef0[k], plan.coef1[k] = coef0[k], coef1[k]
    plan.zeta0, plan.stream0, plan.noise_mode, plan.sample_numel = zeta0, stream0, (1 if zeta0 != 0.0 else 0), sample
    numel = ops[0].numel()
    o = torch.empty(numel, dtype=out, device=DEV)
    _hip.launch_step_masked(plan, on_device(ops), o, mask.to(DEV), mask_numel, batch_stride, seeds.to(DEV) if seeds is not None else None, numel, DEV)
    torch.cuda.synchronize()
    return o.cpu()


# (kernel, tuning switches, three elements more than whole chunks)
STEP_MODES = [("one_trip", {}, False), ("grid_stride", {"one_trip": 0}, False), ("ragged", {}, True)]
FP32_MODES = STEP_MODES + [("no_tile", {"tile": 0}, False), ("grid_stride_no_tile", {"one_trip": 0, "tile": 0}, False)]


def shaped(t, rag):
    return BC.ragged(t) if rag else t


def check_step(ops, coefs, out, what, modes):
    "one output in every mode; the model is elementwise, so the ragged launch's reference is the whole one's with the same three elements behind it"
    want = BM.step(coefs, ops, out=out)
    for mode, switches, rag in modes:
        with tuning(**switches):
            (got,) = launch([shaped(t, rag) for t in ops], coefs, out)
        BM.same_bits(got, shaped(want, rag), operands=[shaped(t, rag) for t in ops], what=f"{what} {mode}")


# ---- skr_step_launch, one output ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.NARROW)
def test_step_patterns(name):
    "every bit pattern through coefficient 1 (K = 1), and beside an operand of ones at coefficient 0 (K = 2)"
    dt, p = BC.DTYPES[name], BC.patterns(name)
    check_step([p], [1.0], dt, f"{name} patterns K=1", STEP_MODES)
    check_step([p, torch.ones_like(p)], [1.0, 0.0], dt, f"{name} patterns K=2", STEP_MODES)
    check_step([p], [1.0], torch.float32, f"{name} patterns fp32 out", STEP_MODES[1:])


@pytest.mark.parametrize("name", BC.NARROW)
def test_step_ties(name):
    for k3 in BC.TIE_K3:
        check_step(BC.tie_operands(name), BC.tie_coefs(k3), BC.DTYPES[name], f"{name} ties k3={k3}", STEP_MODES)


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_step_random(name):
    for k in BC.counts("step"):
        check_step(BC.random_operands(name, k), BC.random_coefs(k, "step"), BC.DTYPES[name], f"{name} random K={k}", FP32_MODES if name == "fp32" else STEP_MODES)


def test_step_specials_fp32():
    check_step(BC.specials32(), BC.SPECIAL_COEFS, torch.float32, "fp32 specials", FP32_MODES)
    check_step(BC.specials32()[:1], [1.0], torch.float32, "fp32 specials K=1", FP32_MODES)


# ---- mixed groups ---------------------------------------------------------------------------------------------------------------------
MIXED_MODES = [("whole", {}, False), ("ragged", {}, True)]


@pytest.mark.parametrize("name", BC.NARROW)
def test_mixed_groups_ties(name):
    "u carried as fp32 behind the 16-bit a; 16-bit and fp32 outputs"
    for k3 in BC.TIE_K3:
        for out in (BC.DTYPES[name], torch.float32):
            check_step(BC.tie_operands(name, wide_u=True), BC.tie_coefs(k3), out, f"{name} mixed ties k3={k3} out={out}", MIXED_MODES)


@pytest.mark.parametrize("name", BC.NARROW)
def test_mixed_groups_random(name):
    "16-bit operands and one fp32 operand (normal in two samples, cancelling the others' sum in two), 16-bit and fp32 outputs; 16-bit operands into an fp32 output"
    for k in BC.MIXED_KS:
        ops, coefs = BC.mixed_operands(name, k)
        for out in (BC.DTYPES[name], torch.float32):
            check_step(ops, coefs, out, f"{name} mixed random K={k} out={out}", MIXED_MODES)
    for k in (1, 5, 9):
        check_step(BC.random_operands(name, k), BC.random_coefs(k, "step"), torch.float32, f"{name} random K={k} fp32 out", MIXED_MODES)


# ---- two outputs ----------------------------------------------------------------------------------------------------------------------
TWO_MODES = [("k2", {"two_out": 2}, False), ("general", {"two_out": 0}, False), ("ragged", {}, True)]


def check_two(ops, c0, c1, chain, out0, out1, what, modes=TWO_MODES):
    w0, w1 = BM.step_two(c0, c1, chain, ops, out0=out0, out1=out1)
    for mode, switches, rag in modes:
        with tuning(**switches):
            g0, g1 = launch([shaped(t, rag) for t in ops], c0, out0, c1, chain, out1)
        seen = [shaped(t, rag) for t in ops]
        BM.same_bits(g0, shaped(w0, rag), operands=seen, what=f"{what} {mode} out0")
        BM.same_bits(g1, shaped(w1, rag), operands=seen, what=f"{what} {mode} out1")


def two_out_operands(name, na, nb):
    ops = list(BC.random_operands(name, na, "two"))
    if nb:
        g = torch.Generator().manual_seed(31 * na + nb)
        ops.append(torch.randn(ROWS, generator=g) * 1.5)
    return ops


@pytest.mark.parametrize("name", BC.NARROW)
def test_two_outputs_random(name):
    dt = BC.DTYPES[name]
    for i, (na, nb) in enumerate(BC.TWO_OUT_PAIRS):
        ops = two_out_operands(name, na, nb)
        c0, c1 = BC.random_coefs(na + nb, "two0"), BC.random_coefs(na + nb, "two1")
        check_two(ops, c0, c1, TC.CHAINS[i], torch.float32, dt, f"{name} two outputs {na}+{nb}")
    ops = two_out_operands(name, 4, 0)  # one dtype throughout: the general kernel alone
    check_two(ops, BC.random_coefs(4, "two0"), BC.random_coefs(4, "two1"), TC.CHAINS[4], dt, dt, f"{name} two 16-bit outputs", TWO_MODES[1:])


@pytest.mark.parametrize("name", BC.NARROW)
def test_two_outputs_ties(name):
    """TIES through coef1 with coef0 = 0 and chain = 1 (the chained value is a signed zero), and through the chain: out0 = u, out1 =
    fma(k3, u, a + u/2) -- the last fma in front of the rounding is the chain's, the one the ragged tail of step_kernel once stored through
    a fused multiply-add-and-convert"""
    dt = BC.DTYPES[name]
    ops = BC.tie_operands(name)
    for k3 in BC.TIE_K3:
        check_two(ops, [0.0, 0.0, 0.0], BC.tie_coefs(k3), 1.0, torch.float32, dt, f"{name} two outputs, ties in coef1 k3={k3}")
        if k3 != 0.0:
            check_two(ops, [0.0, 1.0, 0.0], [*BC.TIE_COEFS, 0.0], k3, torch.float32, dt, f"{name} two outputs, ties through the chain k3={k3}")
            check_two(ops, [0.0, 1.0, 0.0], [*BC.TIE_COEFS, 0.0], k3, dt, dt, f"{name} two 16-bit outputs, ties through the chain k3={k3}", TWO_MODES[1:])


# ---- masked ---------------------------------------------------------------------------------------------------------------------------
def masks_for(dt, sample, samples):
    "(mask, mask_numel, batch_stride): one mask element per element and sample; an eighth of a sample, one mask for the whole batch"
    eighth = sample // 8
    return [(BC.soft_mask(dt, samples, sample, 5), sample, sample), (BC.soft_mask(dt, 1, eighth, 6), eighth, 0)]


def check_masked(ops, c0, c1, mask, mask_numel, stride, out, sample, what, modes):
    samples = ops[0].numel() // sample
    m = BC.expand_mask(mask, stride, samples, sample)
    want = BM.masked(c0, c1, ops, m, out=out)
    for mode, switches in modes:
        with tuning(**switches):
            got = launch_masked(ops, c0, c1, mask, mask_numel, stride, out, sample)
        BM.same_bits(got, want, operands=[m, *ops], what=f"{what} {mode}")


MASKED_MODES = [("v1", {}), ("general", {"one_trip": 0})]


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_masked_random(name):
    dt = BC.DTYPES[name]
    for k in BC.counts("masked"):
        ops, c0, c1 = BC.random_operands(name, k), BC.random_coefs(k, "masked0"), BC.masked_coef1(k)
        for mask, mask_numel, stride in masks_for(dt, BC.SAMPLE, BC.SAMPLES):
            check_masked(ops, c0, c1, mask, mask_numel, stride, dt, BC.SAMPLE, f"{name} masked K={k} mask_numel={mask_numel}", MASKED_MODES)
    # ragged samples (the general kernel): 6140 elements each, a mask of a quarter of that
    k, sample = 5, BC.SAMPLE - 4
    ops = [t[: BC.SAMPLES * sample] for t in BC.random_operands(name, k)]
    for mask, mask_numel, stride in [(BC.soft_mask(dt, BC.SAMPLES, sample, 7), sample, sample), (BC.soft_mask(dt, 1, sample // 4, 8), sample // 4, 0)]:
        check_masked(ops, BC.random_coefs(k, "masked0"), BC.masked_coef1(k), mask, mask_numel, stride, dt, sample, f"{name} masked ragged mask_numel={mask_numel}", [("general", {})])
    if name == "fp32":  # the specials under a soft mask (one sample of one chunk); fp32 operands under a 16-bit mask: the general kernel
        mask = BC.soft_mask(dt, 1, BC.CHUNK, 9)
        check_masked(BC.specials32(), BC.SPECIAL_COEFS, [1.0, -0.75], mask, BC.CHUNK, BC.CHUNK, dt, BC.CHUNK, "fp32 masked specials", MASKED_MODES)
        for mdt in (torch.bfloat16, torch.float16):
            mask, mask_numel, stride = masks_for(mdt, BC.SAMPLE, BC.SAMPLES)[0]
            check_masked(BC.random_operands(name, 5), BC.random_coefs(5, "masked0"), BC.masked_coef1(5), mask, mask_numel, stride, dt, BC.SAMPLE, f"fp32 masked under a {mdt} mask", [("general", {})])
    else:  # the cancelling blend: 16-bit operands, one fp32 operand in the known form, a 16-bit mask and output (the general kernel)
        mask, mask_numel, stride = masks_for(dt, BC.SAMPLE, BC.SAMPLES)[0]
        for k in BC.MIXED_KS:
            ops, c0, c1 = BC.masked_cancelling(name, k, BC.expand_mask(mask, stride, BC.SAMPLES, BC.SAMPLE))
            check_masked(ops, c0, c1, mask, mask_numel, stride, dt, BC.SAMPLE, f"{name} masked cancelling K={k}", [("general", {})])


@pytest.mark.parametrize("name", BC.NARROW)
def test_masked_ties(name):
    "TIES in s under m = 1, in k under m = 0, and s = k under m = 0.5, which rounds once through the last fma; one sample, a mask of 8 equal elements"
    dt = BC.DTYPES[name]
    ops = BC.tie_operands(name)
    numel = ops[0].numel()
    for k3 in BC.TIE_K3:
        tie = BC.tie_coefs(k3)
        for m, c0, c1 in ((1.0, tie, [0.0, 0.0, 1.0]), (0.0, [1.0, 0.0, 0.0], tie), (0.5, tie, tie)):
            mask = torch.full((1, 8), m, dtype=dt)
            check_masked(ops, c0, c1, mask, 8, 0, dt, numel, f"{name} masked ties k3={k3} m={m}", MASKED_MODES)


# ---- backward -------------------------------------------------------------------------------------------------------------------------
BWD_MODES = [("one_trip", {}, False), ("general", {"one_trip": 0}, False), ("ragged", {}, True)]


def check_backward(g0, g1, a, b, dt, what, modes=BWD_MODES):
    wants = [BM.backward(a[k], b[k], g0, g1, out=dt) for k in range(len(a))]
    for mode, switches, rag in modes:
        d0, d1 = shaped(g0, rag).to(DEV), (shaped(g1, rag).to(DEV) if g1 is not None else None)
        with tuning(**switches):
            grads = lazy.launch_backward(d0, d1, a, b, [d0] * len(a), False)
        torch.cuda.synchronize()
        for k, got in enumerate(grads):
            BM.same_bits(got.cpu(), shaped(wants[k], rag), operands=[shaped(g0, rag)] + ([shaped(g1, rag)] if g1 is not None else []), what=f"{what} {mode} grad {k}")


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_backward_random(name):
    dt = BC.DTYPES[name]
    g0, g1 = BC.random_operands(name, 2, "grad")
    for k in BC.counts("backward"):
        a, b = BC.random_coefs(k, "bwd_a"), BC.random_coefs(k, "bwd_b")
        check_backward(g0, None, a, b, dt, f"{name} backward K={k} one gradient")
        check_backward(g0, g1, a, b, dt, f"{name} backward K={k} two gradients")
    if name == "fp32":
        x0, x1 = BC.specials32()
        check_backward(x0, None, [1.0, *BC.SPECIAL_COEFS], [0.0] * 3, dt, "fp32 backward specials one gradient")
        check_backward(x0, x1, [1.0, *BC.SPECIAL_COEFS], [-0.75, 3.0, 1.0], dt, "fp32 backward specials two gradients")


@pytest.mark.parametrize("name", BC.NARROW)
def test_backward_patterns(name):
    "every bit pattern as g0 under a = 1 (and -1, 0.5, 0): mul(1, x) keeps every pattern but the NaNs' payloads"
    p = BC.patterns(name)
    check_backward(p, None, [1.0, -1.0, 0.5, 0.0], [0.0] * 4, BC.DTYPES[name], f"{name} backward patterns")
    check_backward(p, torch.ones_like(p), [1.0, -1.0, 0.5], [0.0, -0.0, 2.0**-9], BC.DTYPES[name], f"{name} backward patterns two gradients")


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_masked_backward_random(name):
    dt = BC.DTYPES[name]
    (g,) = BC.random_operands(name, 1, "grad")
    cases = [(g, BC.SAMPLE, masks_for(dt, BC.SAMPLE, BC.SAMPLES), [("one_trip", {}), ("general", {"one_trip": 0})])]
    sample = BC.SAMPLE - 4  # ragged samples: the general kernel
    cases.append((g[: BC.SAMPLES * sample], sample, [(BC.soft_mask(dt, BC.SAMPLES, sample, 7), sample, sample), (BC.soft_mask(dt, 1, sample // 4, 8), sample // 4, 0)], [("general", {})]))
    if name == "fp32":  # the specials as the incoming gradient: one sample of one chunk
        cases.append((BC.specials32()[0], BC.CHUNK, [(BC.soft_mask(dt, 1, BC.CHUNK, 9), BC.CHUNK, BC.CHUNK)], [("one_trip", {}), ("general", {"one_trip": 0})]))
    for grad, smp, masks, modes in cases:
        for k in BC.counts("masked_backward"):
            a, b = BC.random_coefs(k, "bwd_a"), BC.masked_coef1(k)
            for mask, mask_numel, stride in masks:
                m = BC.expand_mask(mask, stride, grad.numel() // smp, smp)
                wants = [BM.masked_backward(a[j], b[j], m, grad, out=dt) for j in range(k)]
                for mode, switches in modes:
                    d = grad.to(DEV)
                    with tuning(**switches):
                        grads = lazy.launch_masked_backward(d, mask.to(DEV), mask_numel, stride, a, b, [d] * k, smp, False)
                    torch.cuda.synchronize()
                    for j, got in enumerate(grads):
                        BM.same_bits(got.cpu(), wants[j], operands=[m, grad], what=f"{name} masked backward K={k} sample={smp} mask_numel={mask_numel} {mode} grad {j}")


# ---- in-kernel noise ------------------------------------------------------------------------------------------------------------------
SEEDS = TC.seeds_for(BC.SAMPLES)
_z_cache = {}


def extract_z(stream, sample=BC.SAMPLE, numel=ROWS, **switches):
    """the normals a launch of `numel` elements in samples of `sample` draws from `stream` under the seeds TC.seeds_for(numel // sample)
    (ROWS elements in samples of BC.SAMPLE: SEEDS): an fp32 launch over zeros at coefficient 0 with zeta0 = 1"""
    key = (stream, sample, numel, tuple(sorted(switches.items())))
    if key not in _z_cache:
        with tuning(**switches):
            (_z_cache[key],) = launch([torch.zeros(numel)], [0.0], torch.float32, zeta0=1.0, stream0=stream, seeds=TC.seeds_tensor(TC.seeds_for(numel // sample)), sample=sample)
    return _z_cache[key]


PATTERNS3 = 65536 // BC.SAMPLE * BC.SAMPLE  # the patterns in samples of three chunks: the first 61 440
STAGE_GEOMETRIES = ((BC.CHUNK, ROWS), (BC.CHUNK, BC.CHUNK), (BC.CHUNK, 65536), (BC.SAMPLE, PATTERNS3))  # (sample, numel) beside (BC.SAMPLE, ROWS)


def test_the_extracted_normals_are_anchored():
    for stream in TC.STREAMS[:3]:
        z = extract_z(stream)
        for switches in ({"one_trip": 0}, {"tile": 0}, {"one_trip": 0, "tile": 0}):
            BM.same_bits(extract_z(stream, **switches), z, what=f"normals of stream {stream} under {switches}")
        ref = np.concatenate([ON.philox_normal(s, stream, BC.SAMPLE) for s in SEEDS])
        worst = float(np.abs(z.double().numpy() - ref).max())
        print(f"stream {stream}: device normal - oracle normal, worst {worst:.3g} (bar {TC.NORMAL_BAR})")
        assert worst <= TC.NORMAL_BAR, (stream, worst)
    # the geometries of the noisy stage launches: samples of one chunk, and the 65 536 patterns in samples of one and of three chunks
    stream = TC.STREAMS[1]
    for sample, numel in STAGE_GEOMETRIES:
        z = extract_z(stream, sample, numel)
        for switches in ({"one_trip": 0}, {"tile": 0}):
            BM.same_bits(extract_z(stream, sample, numel, **switches), z, what=f"normals of stream {stream}, samples of {sample} in {numel}, under {switches}")
        ref = np.concatenate([ON.philox_normal(s, stream, sample) for s in TC.seeds_for(numel // sample)])
        worst = float(np.abs(z.double().numpy() - ref).max())
        print(f"stream {stream}, samples of {sample} in {numel}: device normal - oracle normal, worst {worst:.3g} (bar {TC.NORMAL_BAR})")
        assert worst <= TC.NORMAL_BAR, (stream, sample, numel, worst)


def check_noisy(got, model, z, what, operands=()):
    """`got` has the bits of model(z), z the normals an fp32 launch of the same geometry, seeds and stream returned.  (On the MI355X every
    16-bit instantiation draws the fp32 launch's normals to the bit: no element needs a neighbour of z, and none is accepted.)"""
    BM.same_bits(got, model(z), operands=operands, what=what)


NOISE = [(TC.ZETAS[0], TC.STREAMS[0]), (TC.ZETAS[2], TC.STREAMS[1])]
NOISY_STEP_MODES = [("one_trip", {}), ("grid_stride", {"one_trip": 0})]


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_noisy_step(name):
    dt = BC.DTYPES[name]
    seeds = TC.seeds_tensor(SEEDS)
    for zeta, stream in NOISE:
        z = extract_z(stream)
        for k in (1, 4, 5, 9, 21):
            ops, coefs = BC.random_operands(name, k), BC.random_coefs(k, "step")
            for mode, switches in NOISY_STEP_MODES + ([("no_tile", {"tile": 0})] if name == "fp32" else []):
                with tuning(**switches):
                    (got,) = launch(ops, coefs, dt, zeta0=zeta, stream0=stream, seeds=seeds, sample=BC.SAMPLE)
                check_noisy(got, lambda zz: BM.step(coefs, ops, zeta, zz, out=dt), z, f"{name} noisy step K={k} zeta={zeta} {mode}", ops)
        if name != "fp32":  # mixed groups, the fp32 operand cancelling the others' sum and the noise
            for k in BC.MIXED_KS:
                ops, coefs = BC.mixed_operands(name, k, zeta, z)
                for out in (dt, torch.float32):
                    (got,) = launch(ops, coefs, out, zeta0=zeta, stream0=stream, seeds=seeds, sample=BC.SAMPLE)
                    check_noisy(got, lambda zz: BM.step(coefs, ops, zeta, zz, out=out), z, f"{name} noisy mixed K={k} zeta={zeta} out={out}", ops)


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_noisy_masked(name):
    dt = BC.DTYPES[name]
    seeds = TC.seeds_tensor(SEEDS)
    for zeta, stream in NOISE:
        z = extract_z(stream)
        for k in (1, 5, 9):
            ops, c0, c1 = BC.random_operands(name, k), BC.random_coefs(k, "masked0"), BC.masked_coef1(k)
            for mask, mask_numel, stride in masks_for(dt, BC.SAMPLE, BC.SAMPLES):
                m = BC.expand_mask(mask, stride, BC.SAMPLES, BC.SAMPLE)
                for mode, switches in MASKED_MODES:
                    with tuning(**switches):
                        got = launch_masked(ops, c0, c1, mask, mask_numel, stride, dt, BC.SAMPLE, zeta, stream, seeds)
                    check_noisy(got, lambda zz: BM.masked(c0, c1, ops, m, zeta, zz, out=dt), z, f"{name} noisy masked K={k} zeta={zeta} mask_numel={mask_numel} {mode}", [m, *ops])


@pytest.mark.parametrize("name", BC.NARROW)
def test_noisy_two_outputs(name):
    "both draws, and each alone; step_kernel_k2 and the general kernel"
    dt = BC.DTYPES[name]
    seeds = TC.seeds_tensor(SEEDS)
    s0, s1 = TC.STREAMS[0], TC.STREAMS[1]
    z0, z1 = extract_z(s0), extract_z(s1)
    for i, (na, nb) in enumerate(BC.TWO_OUT_PAIRS):
        ops = two_out_operands(name, na, nb)
        c0, c1, chain = BC.random_coefs(na + nb, "two0"), BC.random_coefs(na + nb, "two1"), TC.CHAINS[i]
        for zeta0, zeta1 in ((TC.ZETAS[0], TC.ZETAS[2]), (TC.ZETAS[4], 0.0), (0.0, TC.ZETAS[3])):
            for mode, switches in (("k2", {"two_out": 2}), ("general", {"two_out": 0})):
                with tuning(**switches):
                    g0, g1 = launch(ops, c0, torch.float32, c1, chain, dt, zeta0, s0, zeta1, s1, seeds, BC.SAMPLE)
                what = f"{name} noisy two outputs {na}+{nb} zetas=({zeta0}, {zeta1}) {mode}"
                BM.same_bits(g0, BM.step_two(c0, c1, chain, ops, zeta0, z0, zeta1, z1, torch.float32, dt)[0], operands=ops, what=what + " out0")
                check_noisy(g1, lambda zz: BM.step_two(c0, c1, chain, ops, zeta0, z0, zeta1, zz, torch.float32, dt)[1], z1, what + " out1", ops)


# ---- Runge-Kutta stage launches -------------------------------------------------------------------------------------------------------
# out0 = convert_rounded(in[0], in[1]), out1 = sum c1[k] in_k + chain * out0 (+ zeta1 z) against bit_model.rk_stage, both outputs over all
# elements.  Which kernel a launch reaches (launch, launch_rk of skr_step.hip; launch_one_trip_rk, one_trip_ok of skr_step_fast.hip):
#
#   step_kernel_rk1<BLK>    uniform dtype in and out, 2 <= n_terms <= 8, numel % 2048 == 0, "one_trip" on (fp32: "tile" on too);
#                           BLK = 128 when "rk_blk" == 128 or ("rk_blk" == 0 and n_terms <= 6), else 256; with noise: zeta0 == 0 and
#                           sample_numel % 2048 == 0 -- bps_shift >= 0 for a power-of-two number of chunks per sample, else the dividing form
#   step_kernel_rk<UV>      the same launches without noise when the one-trip kernel is not taken: "one_trip" 0, or numel % 8 == 0 and
#                           numel % 2048 != 0 with every switch at its default, or fp32 with "tile" 0; UV = "rk_uv" (0: 1);
#                           fp32 in the tile layout when "tile" is on and numel % 512 == 0
#   step_kernel<..., CONV>  everything else: numel % 8 != 0 (vector body and the scalar tail of store_scalar), n_terms > 8, an fp32
#                           operand behind a 16-bit pair, an fp32 out1 beside 16-bit operands, noise with "one_trip" 0, acc_f64
#
# The table forms of step_kernel_rk1 need no cases here: tests/test_table_forms_gpu.py holds every table instantiation bit for bit to the
# narrow launch (skr_step_launch) of the row's scalars, and the narrow launch is what this file puts under the model.
# acc_f64 launches: out0 alone is claimed (convert in the operands' dtype, or in float64 for fp64 operands); out1 needs an exact float64 fma.

@dataclass(frozen=True)
class Stage:
    what: str
    ops: tuple
    coef1: tuple
    chain: float
    kinds: tuple
    k: tuple
    zeta1: float = 0.0


def launch_stage(dev_ops, c, out1=None, stream1=0, seeds=None, sample=None, acc_f64=False, noisy=False):
    "one skr_step_launch with a rounded conversion over operands on the device; (out0, out1) on the host"
    n, da = len(dev_ops), dev_ops[0].dtype
    na = next((j for j, t in enumerate(dev_ops) if t.dtype != da), n)
    numel = dev_ops[0].numel()
    assert all(t.numel() == numel and t.is_contiguous() for t in dev_ops) and all(t.dtype == dev_ops[-1].dtype for t in dev_ops[na:])
    plan = _hip.StepPlanC()
    plan.n_terms, plan.n_group_a, plan.dtype_a = n, na, CODE[da]
    plan.dtype_b = CODE[dev_ops[-1].dtype] if na < n else CODE[da]
    plan.out0_dtype, plan.out1_dtype, plan.acc_f64 = CODE[da], CODE[out1 if out1 is not None else da], int(acc_f64)
    for j in range(n):
        plan.coef0[j], plan.coef1[j] = 0.0, c.coef1[j]
    plan.chain, plan.convert_to, plan.convert_from = c.chain, *c.kinds
    for i in range(4):
        plan.convert_k[i] = c.k[i]
    if noisy:
        plan.noise_mode, plan.zeta1, plan.stream1 = 1, c.zeta1, stream1
    plan.sample_numel = sample if sample is not None else numel
    o0 = torch.full((numel,), 7.0, dtype=da, device=DEV)
    o1 = torch.full((numel,), 7.0, dtype=out1 if out1 is not None else da, device=DEV)
    _hip.launch_step(plan, list(dev_ops), o0, o1, seeds.to(DEV) if seeds is not None else None, numel, DEV)
    torch.cuda.synchronize()
    return o0.cpu(), o1.cpu()


# the shapes of a launch over a set of whole chunks (host or device tensors)
SHAPES = {
    "whole": lambda t: t,
    "eights": lambda t: t[: t.numel() - 1032],  # a multiple of 8, not of 512
    "tiles": lambda t: t[: t.numel() - 512],  # a multiple of 512, not of 2048
    "ragged": BC.ragged,  # three elements more than whole chunks
}
RK1_ROUTES = [("rk1 128 threads", {"rk_blk": 128}, "whole"), ("rk1 256 threads", {"rk_blk": 256}, "whole")]
RK_ROUTES = [(f"rk {uv} per lane", {"one_trip": 0, "rk_uv": uv}, "whole") for uv in (1, 2, 4)] + [("rk, all default", {}, "eights"), ("rk 4 per lane, eights", {"rk_uv": 4}, "eights")]
RK_ROUTES32 = [("rk no tile", {"tile": 0}, "whole"), ("rk 2 per lane no tile", {"one_trip": 0, "tile": 0, "rk_uv": 2}, "whole"), ("rk tiles", {}, "tiles"), ("rk 4 per lane tiles", {"rk_uv": 4}, "tiles")]
ONE_TRIP = ("rk1", {}, "whole")
GENERAL = ("general, ragged", {}, "ragged")


def uniform_routes(name):
    return RK1_ROUTES + RK_ROUTES + (RK_ROUTES32 if name == "fp32" else []) + [GENERAL]


_stage_models = {}


def stage_model(c: Stage, out1=None, z1=None, key=None):
    "bit_model.rk_stage of a case, computed once (the model is elementwise: every shape of a launch is a slice of it)"
    key = (c.what, out1, key)
    if key not in _stage_models:
        assert (z1 is None) == (key[2] is None)
        _stage_models[key] = BM.rk_stage(c.coef1, c.chain, c.ops, c.kinds, c.k, c.zeta1 if z1 is not None else None, z1, out=out1)
    return _stage_models[key]


def check_stage(c: Stage, routes, out1=None):
    w0, w1 = stage_model(c, out1)
    dev = on_device(c.ops)
    for label, switches, shape in routes:
        cut = SHAPES[shape]
        with tuning(**switches):
            g0, g1 = launch_stage([cut(t).contiguous() for t in dev], c, out1)
        seen = [cut(t) for t in c.ops]
        BM.same_bits(g0, cut(w0), operands=seen, what=f"{c.what}, {label}: out0")
        BM.same_bits(g1, cut(w1), operands=seen, what=f"{c.what}, {label}: out1")


def conversion_stages(name, pairs, k_sets=None, operands=None):
    """the dtype's conversion inputs (BC.conversion_inputs) as stage launches: per input, k set and kinds pair one case; K runs over
    BC.STAGE_KS with the case, seeded normals behind the pair, coef1 as BC.random_coefs, the chains of table_cases.CHAINS.
    operands(pair, K) -> (operands, what) builds another operand list around the pair."""
    out = []
    for i, (what, s, o, ks) in enumerate(BC.conversion_inputs(name)):
        for j, k in enumerate(ks):
            if k_sets is not None and j not in k_sets:
                continue
            for kinds in pairs:
                at = 4 * kinds[0] + kinds[1] + i + j
                K = BC.STAGE_KS[at % len(BC.STAGE_KS)]
                ops, how = operands((s, o), K) if operands is not None else (BC.stage_operands(name, (s, o), K), f"K={K}")
                out.append(Stage(f"{name} {what} kinds={kinds} k[{j}] {how}", tuple(ops), tuple(BC.stage_coefs(len(ops))), TC.CHAINS[at % len(TC.CHAINS)], kinds, k))
    return out


def cancelling_stages(name, Ks=BC.STAGE_KS, last=None):
    "BC.stage_cancelling at every K, under kinds (1, 2) and one of BC.KINDS_FIVE; last(s) -> the last operand in another dtype"
    out = []
    for i, K in enumerate(Ks):
        ops, coefs, chain, zeta1 = BC.stage_cancelling(name, K)
        if last is not None:
            ops = (*ops[:-1], last(ops[-1]))
        for kinds in ((1, 2), BC.KINDS_FIVE[i % len(BC.KINDS_FIVE)]):
            out.append(Stage(f"{name} cancelling K={K} kinds={kinds}{'' if last is None else ' wide last'}", ops, tuple(coefs), chain, kinds, BC.CONVERT_KS[i % 2], zeta1))
    return out


REST = [kd for kd in BC.KINDS if kd not in BC.KINDS_FIVE]


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_stage_conversion(name):
    """16-bit: every bit pattern as s against a permutation as o and the reverse; fp32: normals, and the specials block (with k that
    overflow products and underflow quotients).  All 15 kinds pairs through the one-trip kernel and the general kernel's ragged launch,
    the five pairs that hold every operation through every other route."""
    for c in conversion_stages(name, BC.KINDS_FIVE):
        check_stage(c, uniform_routes(name))
    for c in conversion_stages(name, REST):
        check_stage(c, [ONE_TRIP, GENERAL])


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_stage_cancelling(name):
    "the self-cancelling s at K = 2, 4, 5, 8 through every route: the order of the operands, the place of the chain, whole fmas"
    for c in cancelling_stages(name):
        check_stage(c, uniform_routes(name))


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_stage_general_kernel_launches(name):
    """step_kernel<..., CONV> on the launches no stage kernel takes: nine operands (whole chunks: the vector body alone; fp32 with and
    without the tile layout); a 16-bit pair with one fp32 operand behind it; an fp32 out1 beside 16-bit operands"""
    both = [("general", {}, "whole"), GENERAL]
    nine = both + ([("general no tile", {"tile": 0}, "whole")] if name == "fp32" else [])
    many = lambda pair, K: (BC.stage_operands(name, pair, 9), "K=9")  # noqa: E731
    for c in conversion_stages(name, BC.KINDS_FIVE, operands=many) + cancelling_stages(name, Ks=(9,)):
        check_stage(c, nine)
    if name == "fp32":
        return
    wide = lambda pair, K: ((*pair, BC.stage_extras("fp32", pair[0].numel())[0]), "fp32 operand")  # noqa: E731
    for c in conversion_stages(name, BC.KINDS_FIVE, operands=wide) + cancelling_stages(name, Ks=(3, 5), last=lambda s: s.float()):
        check_stage(c, both)
    for c in conversion_stages(name, BC.KINDS_FIVE, k_sets=(0,)) + cancelling_stages(name, Ks=(2, 5)):
        check_stage(c, both, out1=torch.float32)


def noisy_stage_cases(name, sample):
    "(case, numel): the chain as the canceller and the self-cancelling s (ROWS elements); the conversion inputs under the first k set"
    ops, coefs, chain, zeta1, kinds, k = BC.stage_chain_cancels(name)
    cases = [Stage(f"{name} chain cancels", ops, tuple(coefs), chain, kinds, k, zeta1)] + cancelling_stages(name, Ks=(2, 5))
    for c in conversion_stages(name, BC.KINDS_FIVE, k_sets=(0,)):
        cases.append(Stage(c.what, c.ops, c.coef1, c.chain, c.kinds, c.k, TC.ZETAS[2]))
    return [c for c in cases if c.ops[0].numel() // sample * sample > 0]


@pytest.mark.parametrize("sample", (BC.CHUNK, BC.SAMPLE))
@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_noisy_stage(name, sample):
    """the last stage of a stochastic step: zeta1 != 0, the draw on out1 alone.  Samples of one chunk (chunk -> sample by a shift) and of
    three (by a division), step_kernel_rk1 at both block sizes and the general kernel ("one_trip" 0; fp32 also without the tile layout)"""
    stream = TC.STREAMS[1]
    routes = [(label, switches) for label, switches, _ in RK1_ROUTES] + [("general", {"one_trip": 0})] + ([("general no tile", {"tile": 0})] if name == "fp32" else [])
    for c in noisy_stage_cases(name, sample):
        numel = c.ops[0].numel() // sample * sample
        z1 = extract_z(stream, sample, numel)
        seeds = TC.seeds_tensor(TC.seeds_for(numel // sample))
        cut = Stage(c.what, tuple(t[:numel] for t in c.ops), c.coef1, c.chain, c.kinds, c.k, c.zeta1)
        w0, w1 = stage_model(cut, None, z1, key=(sample, numel))
        dev = on_device(cut.ops)
        for label, switches in routes:
            with tuning(**switches):
                g0, g1 = launch_stage(dev, cut, None, stream, seeds, sample, noisy=True)
            BM.same_bits(g0, w0, operands=cut.ops, what=f"{c.what}, noisy, samples of {sample}, {label}: out0")
            BM.same_bits(g1, w1, operands=cut.ops, what=f"{c.what}, noisy, samples of {sample}, {label}: out1")


@pytest.mark.parametrize("name", BC.STAGE_DTYPES)
def test_stage_acc_f64_derivative(name):
    """acc_f64 launches (the general kernel, float64 sums): out0 is the conversion in the operands' dtype -- convert_rounded in fp32 with
    both roundings for 16-bit and fp32 operands, in float64 for fp64 operands -- on whole chunks and three elements more.  out1 is not
    compared (the float64 sum needs a model of its own)."""
    dt = BC.STAGE_DTYPES[name]
    for what, s, o, ks in BC.conversion_inputs(name):
        extras = [t.to(dt) for t in BC.stage_extras("fp32" if name == "fp64" else name, s.numel())[:3]]
        dev = on_device([s, o, *extras])
        for j, k in enumerate(ks):
            for kinds in BC.KINDS_FIVE:
                want = BM.convert(dt, s, o, kinds, k)
                for K in (2, 5):
                    c = Stage(f"{name} acc_f64 {what} kinds={kinds} k[{j}] K={K}", (), tuple(BC.stage_coefs(K)), TC.CHAINS[j], kinds, k)
                    for label, shape in (("whole", "whole"), ("ragged", "ragged")):
                        g0, _ = launch_stage([SHAPES[shape](t).contiguous() for t in dev[:K]], c, acc_f64=True)
                        BM.same_bits(g0, SHAPES[shape](want), operands=[SHAPES[shape](s), SHAPES[shape](o)], what=f"{c.what} {label}: out0")
