"""The host executors of lazy.error_mean and lazy.power_blend (CPU tensors and ndarrays) against the references and the derived bars
of reduce_cases.py -- the ones the device kernels are held to in test_reduce_gpu.py.  No GPU."""

import numpy as np
import pytest
import reduce_cases as RC
import torch

from skrample_amd.sampling import lazy

HOST_NORM_SIZES = [n for n in RC.NORM_SIZES if n <= 3000]


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.NAME.get)
def test_error_mean_host(dtype):
    for numel in HOST_NORM_SIZES:
        a, b = RC.norm_inputs(numel, dtype, seed=numel)
        for power in (1, 2):
            for lhs in (a, 0):
                exact = RC.norm_exact(a if lhs is a else None, b, power)
                bar = RC.norm_bar(numel) * exact
                got = lazy.error_mean(lhs, b, power)
                assert isinstance(got, float) and abs(got - exact) <= bar, (numel, power, got, exact)
                if numel in RC.NORM_EXACT_SIZES:
                    frac = RC.norm_fraction(a if lhs is a else None, b, power)
                    assert abs(float(got - frac)) <= RC.norm_bar(numel) * float(frac), (numel, power, got, float(frac))
                if dtype != torch.bfloat16:  # (numpy has no bfloat16)
                    got_np = lazy.error_mean(lhs.numpy() if lhs is a else 0, b.numpy(), power)
                    assert abs(got_np - exact) <= bar, (numel, power, got_np, exact)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.NAME.get)
def test_error_mean_host_edges(dtype):
    a, b = RC.norm_inputs(100, dtype, seed=5)
    for power in (1, 2):
        for value, check in ((float("inf"), lambda v: v == float("inf")), (float("nan"), lambda v: v != v)):
            bad = b.clone()
            bad[37] = value
            assert check(lazy.error_mean(a, bad, power)) and check(lazy.error_mean(0, bad, power)), (power, value)
        if dtype != torch.float64:
            tiny = RC.subnormals(dtype)
            for lhs in (None, tiny.flip(0)):
                exact = RC.norm_exact(lhs, tiny, power)
                assert exact > 0 and abs(lazy.error_mean(0 if lhs is None else lhs, tiny, power) - exact) <= RC.norm_bar(tiny.numel()) * exact
    m = a.reshape(4, 25)
    assert lazy.error_mean(m.t(), b.reshape(4, 25).t(), 2) == lazy.error_mean(m.t().contiguous(), b.reshape(4, 25).t().contiguous(), 2)


HOST_PAIRS = [(torch.float32, torch.float32, torch.float32), (torch.float64, torch.float64, torch.float64), (torch.bfloat16, torch.float32, torch.float32)]


@pytest.mark.parametrize("power", RC.BLEND_POWERS)
@pytest.mark.parametrize("pair", HOST_PAIRS, ids=lambda p: "x".join(RC.NAME[d] for d in p))
def test_power_blend_host(pair, power):
    a_dtype, c_dtype, result = pair
    for k, (wp, wc) in enumerate(RC.WEIGHTS):
        for cancel in (False, True):
            a, c = RC.blend_inputs(RC.BLEND_N, 7100 + 2 * k + cancel, power, wp, wc, cancel, a_dtype, c_dtype)
            ref = RC.BlendRef(a, c, wp, wc, power, result)
            got = lazy.power_blend(a, c, wp, wc, power, result)
            assert got.dtype == result and got.shape == a.shape
            assert ref.margin(got) < 1.0, (pair, power, wp, cancel, ref.margin(got))
            assert ref.margin(RC.blend_torch(a, c, wp, wc, power, result)) < 1.0
            if a_dtype != torch.bfloat16:
                got_np = lazy.power_blend(a.numpy(), c.numpy(), wp, wc, power, result)
                assert isinstance(got_np, np.ndarray) and np.array_equal(got_np, got.numpy())


@pytest.mark.parametrize("power", [2.0, 0.5, -1.0])
@pytest.mark.parametrize("result", [torch.float32, torch.float64], ids=RC.NAME.get)
def test_power_blend_host_zeros_signs_nonfinite(result, power):
    """The header's definition: sign(0) = sign(-0) = +1, so |0|^-1 blends to +inf (a sign() that is 0 at 0 gives NaN there).  Exact
    cancellation (a = -b, equal weights) makes the inner sum an exact zero."""
    for operand in (result, torch.float16):
        a, c = RC.special_pairs(operand)
        for wp, wc in ((0.5, 0.5), RC.WEIGHTS[1]):
            want = RC.blend_torch(a, c, wp, wc, power, result)
            for got in (lazy.power_blend(a, c, wp, wc, power, result), torch.from_numpy(lazy.power_blend(a.numpy(), c.numpy(), wp, wc, power, result))):
                RC.assert_same_specials(got, want, (power, wp))
                assert RC.BlendRef(a, c, wp, wc, power, result).margin(got) < 1.0
    zero = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=result)
    other = torch.tensor([0.0, 0.0, 1.5, -1.5], dtype=result)
    got = lazy.power_blend(zero, other, 0.5, 0.5, -1.0, result)
    assert got.tolist() == [0.0, 0.0, 0.0, 0.0] and not torch.signbit(got).any()  # 1 / (inf + ...) = +0: every |0|^-1 is +inf
    assert lazy.power_blend(zero, -zero, 0.5, 0.5, 2.0, result).tolist() == [0.0] * 4
    assert torch.equal(lazy.power_blend(torch.tensor([1.5, -1.5], dtype=result), torch.tensor([-1.5, 1.5], dtype=result), 0.5, 0.5, -1.0, result), torch.tensor([float("inf")] * 2, dtype=result))


@pytest.mark.parametrize("power", [2.0, 0.5, 1.0, 3.0])
@pytest.mark.parametrize("arith", [torch.float32, torch.float64], ids=RC.NAME.get)
def test_power_blend_host_autograd_at_zeros(arith, power):
    """Host autograd at exact zeros: 0 where the exponent is >= 0, NaN where a zero meets a negative one -- what the expression with
    sign(0) = 0 gave as well, since |x|'s own derivative is 0 at 0 either way.  The device's zero tables are compared with this."""
    old = lambda v, f: v.abs().pow(f) * v.sign()  # noqa: E731
    for operand in (arith, torch.bfloat16):
        av, cv = (torch.tensor(col, dtype=operand) for col in RC.ZERO_TABLE)
        ah, ch = av.clone().requires_grad_(), cv.clone().requires_grad_()
        lazy.power_blend(ah, ch, 0.5, 0.5, power, arith).sum().backward()
        ao, co = av.clone().requires_grad_(), cv.clone().requires_grad_()
        old(0.5 * old(ao.to(arith), power) + 0.5 * old(co.to(arith), power), 1 / power).sum().backward()
        for got, want in ((ah.grad, ao.grad), (ch.grad, co.grad)):
            assert got.dtype == operand and torch.equal(torch.isnan(got), torch.isnan(want)), (power, got, want)
            assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want)), (power, got, want)
        ga, gc = RC.blend_grads(av, cv, 0.5, 0.5, power, arith)
        for got, want, x, other in ((ah.grad, ga, av, cv), (ch.grad, gc, cv, av)):
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (power, got, want)
            ok = torch.isfinite(want).numpy()
            bound = RC.grad_bound(want.numpy(), x, 0.5, 0.5, other, power, operand, arith)
            assert (np.abs(got.double().numpy() - want.numpy())[ok] <= bound[ok]).all(), (power, got, want)
