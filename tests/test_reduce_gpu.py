"""skr_reduce.hip on the device: the error norm (skr_error_mean) in every dtype, with and without `a`, through every size path of
its grid-capped reduction, against an exactly rounded sum; the signed-power blend (skr_power_blend) and its backward in all 32
instantiations each, on the stride path, over a wide dynamic range and at zeros / signs / non-finite values, against the reference
formula evaluated in a wider arithmetic.  References and bars: reduce_cases.py (derived, never measured on the kernels)."""

import itertools

import numpy as np
import pytest
import reduce_cases as RC
import torch
from conftest import note_margin

from skrample_amd import _hip
from skrample_amd._hip import SkrampleHipError
from skrample_amd.sampling import lazy

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
PAIRS = list(itertools.product(RC.DTYPES, RC.DTYPES))


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


# ---- 1. error norm -----------------------------------------------------------------------------------------------------------------
def _norm(lib, ws, a, b, power, numel=None, dtype_code=None):
    "skr_error_mean through ctypes on a caller's workspace (out = ws[0], partials = ws[1:]); NaN-poisoned before every call"
    ws.fill_(float("nan"))
    status = lib.skr_error_mean(a.data_ptr() if a is not None else None, b.data_ptr(), _hip.DTYPE_CODE[b.dtype] if dtype_code is None else dtype_code,
                                b.numel() if numel is None else numel, power, ws.data_ptr(), ws.data_ptr() + 8, _hip.current_stream_ptr(b.device))
    return status, ws[0].item()


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.NAME.get)
def test_error_mean_every_path(dtype, dev):
    "every instantiation (4 dtypes x `a` or NULL), powers 1 and 2, at every size where the reduction takes another path"
    lib = _hip.load()
    ws = torch.empty(1025, dtype=F64, device=dev)
    worst = 0.0
    for numel in RC.NORM_SIZES:
        a, b = RC.norm_inputs(numel, dtype, seed=numel)
        ad, bd = a.to(dev), b.to(dev)
        for power in (1, 2):
            for lhs, lhs_dev in ((a, ad), (None, None)):
                exact = RC.norm_exact(lhs, b, power)
                bar = RC.norm_bar(numel) * exact
                status, got = _norm(lib, ws, lhs_dev, bd, power)
                assert status == 0
                worst = max(worst, abs(got - exact) / bar)
                assert abs(got - exact) <= bar, (numel, power, lhs is None, got, exact, abs(got - exact) / exact)
                assert abs(got - exact) < 1e-12  # the bar of test_rkmoire_on_device
                assert lazy.error_mean(0 if lhs is None else lhs_dev, bd, power) == got, (numel, power)
                if numel in RC.NORM_EXACT_SIZES:
                    frac = RC.norm_fraction(lhs, b, power)
                    assert abs(float(got - frac)) <= RC.norm_bar(numel) * float(frac), (numel, power, got, float(frac))
        if numel == RC.NORM_SIZES[-1]:  # bit-reproducible: the same input gives the same bits, launch after launch
            first = _norm(lib, ws, ad, bd, 2)[1]
            assert all(np.float64(_norm(lib, ws, ad, bd, 2)[1]).tobytes() == np.float64(first).tobytes() for _ in range(3))
    note_margin("reduce", f"error_mean {RC.NAME[dtype]} |got - exact| / bar", worst, 1.0)


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.NAME.get)
def test_error_mean_edge_values(dtype, dev):
    lib = _hip.load()
    ws = torch.empty(1025, dtype=F64, device=dev)
    a, b = RC.norm_inputs(300, dtype, seed=11)
    for power in (1, 2):
        for value, check in ((float("inf"), lambda v: v == float("inf")), (float("-inf"), lambda v: v == float("inf")), (float("nan"), lambda v: v != v)):
            bad = b.clone()
            bad[257] = value
            for lhs in (a.to(dev), None):
                assert check(_norm(lib, ws, lhs, bad.to(dev), power)[1]), (power, value, lhs is None)
        if dtype != F64:  # a tensor of the dtype's subnormals: the exact mean, nothing flushed
            tiny = RC.subnormals(dtype)
            for lhs in (None, tiny.flip(0)):
                exact = RC.norm_exact(lhs, tiny, power)
                got = _norm(lib, ws, None if lhs is None else lhs.to(dev), tiny.to(dev), power)[1]
                assert exact > 0 and abs(got - exact) <= RC.norm_bar(tiny.numel()) * exact, (power, lhs is None, got, exact)
    if dtype == torch.float16:  # the largest fp16 magnitudes: |a - b| = 131008 and its square exist only in the wider arithmetic
        top = torch.full((300,), 65504.0, dtype=dtype)
        top[::3] = -65504.0
        for lhs in (None, -top):
            exact = RC.norm_exact(lhs, top, 2)
            got = _norm(lib, ws, None if lhs is None else lhs.to(dev), top.to(dev), 2)[1]
            assert np.isfinite(got) and abs(got - exact) <= RC.norm_bar(300) * exact, (got, exact)
    # non-contiguous operands
    m, k = a.reshape(12, 25).to(dev), b.reshape(12, 25).to(dev)
    assert lazy.error_mean(m.t(), k.t(), 2) == lazy.error_mean(m.t().contiguous(), k.t().contiguous(), 2) == lazy.error_mean(m, k, 2)
    # operand views (tests/view_cases.py): storage in another axis order, a strided slice and an odd address, each inside a padded base that
    # stays untouched -- the contiguous clones' mean, bit for bit (the kernel reads the normalised copy in logical order)
    import view_cases as VC

    for kind in ("permuted_other", "sliced", "offset_small"):
        for power in (1, 2):
            va, vb = (VC.KINDS[kind](t.reshape(2, 3, 5, 10).to(dev)) for t in (a, b))
            watch = VC.Watch(va, vb)
            assert lazy.error_mean(va, vb, power) == lazy.error_mean(VC.twin(va), VC.twin(vb), power), (kind, power)
            assert lazy.error_mean(0, vb, power) == lazy.error_mean(0, VC.twin(vb), power), (kind, power)
            watch.assert_untouched(f"error_mean {kind}")


def test_error_mean_refusals(dev):
    "refused before any launch: the poisoned workspace is untouched"
    lib = _hip.load()
    ws = torch.empty(1025, dtype=F64, device=dev)
    b = torch.ones(64, device=dev)
    stream = _hip.current_stream_ptr(dev)
    for kwargs, want in ((dict(numel=0), 5), (dict(numel=-1), 5), (dict(power=3), 7), (dict(power=0), 7), (dict(dtype_code=99), 2), (dict(dtype_code=-1), 2)):  # SKR_ERR_SHAPE, _UNSUPPORTED, _DTYPE
        assert _norm(lib, ws, None, b, kwargs.pop("power", 2), **kwargs)[0] == want, (kwargs, want)
        assert torch.isnan(ws).all()
    ws.fill_(float("nan"))
    for args in ((None, None, 2, 64, 2, ws.data_ptr(), ws.data_ptr() + 8), (None, b.data_ptr(), 2, 64, 2, None, ws.data_ptr() + 8), (None, b.data_ptr(), 2, 64, 2, ws.data_ptr(), None)):
        assert lib.skr_error_mean(*args, stream) == 1  # SKR_ERR_NULL
    torch.cuda.synchronize()
    assert torch.isnan(ws).all()
    with pytest.raises(SkrampleHipError, match="dtype and shape"):
        lazy.error_mean(b.half(), b, 2)
    with pytest.raises(SkrampleHipError, match="dtype and shape"):
        lazy.error_mean(b[:32], b, 2)
    with pytest.raises(SkrampleHipError, match="non-zero scalar"):
        lazy.error_mean(0.5, b, 2)
    assert lazy.error_mean(0, b, 2) == 1.0 and lazy.error_mean(0.0, b, 1) == 1.0


# ---- 2. blend forward: all 32 instantiations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", RC.BLEND_POWERS)
@pytest.mark.parametrize("result", [F32, F64], ids=RC.NAME.get)
def test_power_blend_every_instantiation(result, power, dev):
    """Operand dtypes do not enter the bar: the loads are exact widenings, so a 16-bit pair failing where f32 x f32 passes is a load
    bug.  torch's own CPU evaluation in the result arithmetic sits under the same bound (the bound is not vacuous)."""
    worst, worst_torch = 0.0, 0.0
    for a_dtype, c_dtype in PAIRS:
        for k, (wp, wc) in enumerate(RC.WEIGHTS):
            for cancel in (False, True):
                a, c = RC.blend_inputs(RC.BLEND_N, 7100 + 2 * k + cancel, power, wp, wc, cancel, a_dtype, c_dtype)
                ref = RC.BlendRef(a, c, wp, wc, power, result)
                got = lazy.power_blend(a.to(dev), c.to(dev), wp, wc, power, result)
                assert got.dtype == result and got.shape == a.shape
                margin, margin_torch = ref.margin(got), ref.margin(RC.blend_torch(a, c, wp, wc, power, result))
                assert margin < 1.0, (RC.NAME[a_dtype], RC.NAME[c_dtype], power, wp, cancel, margin)
                assert margin_torch < 1.0, (RC.NAME[a_dtype], RC.NAME[c_dtype], power, wp, cancel, margin_torch)
                worst, worst_torch = max(worst, margin), max(worst_torch, margin_torch)
    note_margin("reduce", f"power_blend -> {RC.NAME[result]} P={power:.3g} device err / bound", worst, 1.0)
    note_margin("reduce", f"power_blend -> {RC.NAME[result]} P={power:.3g} torch-cpu err / bound", worst_torch, 1.0)


# ---- 3. blend forward: the stride path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(F32, F32), (torch.bfloat16, torch.float16)], ids=lambda p: "x".join(RC.NAME[d] for d in p))
def test_power_blend_stride_path(pair, dev):
    "more elements than the capped grid has lanes: the first 4099 lanes take a second trip; elementwise results cannot depend on the grid"
    whole = RC.BLEND_STRIDE_BLOCKS * 256
    n, (wp, wc) = whole + 4099, RC.WEIGHTS[0]
    a, c = RC.blend_inputs(n, 7300, 2.0, wp, wc, False, *pair)
    ad, cd = a.to(dev), c.to(dev)
    got = lazy.power_blend(ad, cd, wp, wc, 2.0, F32)
    margin = RC.BlendRef(a, c, wp, wc, 2.0, F32).margin(got)
    assert margin < 1.0, margin
    assert torch.equal(got[:whole], lazy.power_blend(ad[:whole], cd[:whole], wp, wc, 2.0, F32))
    assert torch.equal(got[whole:], lazy.power_blend(ad[whole:].clone(), cd[whole:].clone(), wp, wc, 2.0, F32))


# ---- 4. blend forward: wide dynamic range ----------------------------------------------------------------------------------------
# The raw log2 / exp2 units amplify their 1-ULP error by about |f log2|x||, so K = 64 is not a given over the fp16 normal range.
# Measured worst err / (eps32 scale) (RC.BlendRef.units), 16 dtype pairs x 2 weight pairs x 4096 elements, against float64
# (MI355X; profiles/reduce_margins.txt):
#     P       0.5     2       3       1/3     0.75
#     device  12.85   11.41   18.98   17.97   19.55
#     torch   3.50    1.35    3.36    6.51    4.52     (fp32 on the CPU)
# so the asserted bar max(64, 2 x torch-fp32) is 64 for every power: K = 64 holds over the fp16 normal range.
@pytest.mark.parametrize("power", RC.BLEND_POWERS)
def test_power_blend_wide_range(power, dev):
    worst, worst_torch = 0.0, 0.0
    for a_dtype, c_dtype in PAIRS:
        for k, (wp, wc) in enumerate(RC.WEIGHTS):
            g = torch.Generator().manual_seed(7400 + k)
            mag = torch.exp2(torch.rand(2, 4096, generator=g, dtype=F64) * 28 - 14)  # log-uniform over [2^-14, 2^14]
            sign = torch.where(torch.rand(2, 4096, generator=g) < 0.5, -1.0, 1.0).double()
            a, c = (mag[0] * sign[0]).to(a_dtype), (mag[1] * sign[1]).to(c_dtype)
            ref = RC.BlendRef(a, c, wp, wc, power, F32)
            worst = max(worst, ref.units(lazy.power_blend(a.to(dev), c.to(dev), wp, wc, power, F32)))
            worst_torch = max(worst_torch, ref.units(RC.blend_torch(a, c, wp, wc, power, F32)))
    bar = max(RC.K, 2.0 * worst_torch)
    note_margin("reduce", f"power_blend wide range P={power:.3g} device err / (eps32 scale)", worst, bar)
    note_margin("reduce", f"power_blend wide range P={power:.3g} torch-cpu fp32 err / (eps32 scale)", worst_torch, bar)
    print(f"wide range P={power:.3g}: device {worst:.2f}, torch fp32 {worst_torch:.2f}, bar {bar:.2f} (units of eps32 * scale)")
    assert worst <= bar, (power, worst, worst_torch, bar)


# ---- 5. blend forward: zeros, signs, non-finite values ---------------------------------------------------------------------------
@pytest.mark.parametrize("power", [2.0, 0.5, -1.0])
@pytest.mark.parametrize("result", [F32, F64], ids=RC.NAME.get)
def test_power_blend_zeros_signs_nonfinite(result, power, dev):
    "all pairs of {+0, -0, +-1.5, +-inf, NaN}, exact cancellation (a = -b, equal weights: u = 0) among them, in every operand dtype"
    for operand in RC.DTYPES:
        a, c = RC.special_pairs(operand)
        for wp, wc in ((0.5, 0.5), RC.WEIGHTS[1]):
            want = RC.blend_torch(a, c, wp, wc, power, result)
            got = lazy.power_blend(a.to(dev), c.to(dev), wp, wc, power, result)
            RC.assert_same_specials(got, want, (RC.NAME[operand], power, wp))
            assert RC.BlendRef(a, c, wp, wc, power, result).margin(got) < 1.0, (RC.NAME[operand], power, wp)


# ---- 6. blend backward: all 32 instantiations ------------------------------------------------------------------------------------
def _device_grads(a, c, wp, wc, power, arith, dev, wants=(True, True)):
    ad, cd = a.clone().to(dev).requires_grad_(wants[0]), c.clone().to(dev).requires_grad_(wants[1])
    lazy.power_blend(ad, cd, wp, wc, power, arith).sum().backward()
    return ad.grad, cd.grad


@pytest.mark.parametrize("power", RC.GRAD_POWERS)
@pytest.mark.parametrize("arith", [F32, F64], ids=RC.NAME.get)
def test_power_blend_backward_every_instantiation(arith, power, dev):
    """Plain randn operands, values near zero included, nothing excluded.  Where the inner sum cancels to within its own rounding and
    P > 1 the gradient has no finite bound (RC.grad_bound); those elements are counted and must stay rare."""
    worst, worst_torch, unbounded, total = 0.0, 0.0, 0, 0
    for a_dtype, c_dtype in PAIRS:
        for k, (wp, wc) in enumerate(RC.WEIGHTS):
            a, c = RC.blend_inputs(RC.BLEND_N, 7600 + k, power, wp, wc, False, a_dtype, c_dtype)
            exact = RC.blend_grads(a, c, wp, wc, power, F64)
            own = RC.blend_grads(a, c, wp, wc, power, arith)  # torch's CPU autograd in the kernel's arithmetic, unrounded
            got = _device_grads(a, c, wp, wc, power, arith, dev)
            assert got[0].dtype == a_dtype and got[1].dtype == c_dtype and got[0].shape == a.shape
            sides = ((a, wp, wc, c), (c, wc, wp, a))
            for side, (x, w, w_other, x_other) in enumerate(sides):
                want = exact[side].numpy()
                bound = RC.grad_bound(want, x, w, w_other, x_other, power, x.dtype, arith)
                err = np.abs(got[side].cpu().double().numpy() - want)
                assert np.isfinite(err).all() and (err <= bound).all(), (RC.NAME[a_dtype], RC.NAME[c_dtype], power, wp, side, float((err / bound).max()))
                finite = np.isfinite(bound)
                unbounded, total = unbounded + int((~finite).sum()), total + bound.size
                worst = max(worst, float((err[finite] / bound[finite]).max()))
                unrounded = RC.grad_bound(want, x, w, w_other, x_other, power, arith, arith)
                worst_torch = max(worst_torch, float((np.abs(own[side].numpy() - want)[finite] / unrounded[finite]).max()))
            # one-sided calls: the same bits as the two-sided call for that operand
            only_a, none_c = _device_grads(a, c, wp, wc, power, arith, dev, (True, False))
            none_a, only_c = _device_grads(a, c, wp, wc, power, arith, dev, (False, True))
            assert none_a is None and none_c is None
            assert torch.equal(only_a, got[0]) and torch.equal(only_c, got[1])
    assert unbounded <= total // 100, (unbounded, total)
    assert worst_torch < 1.0, worst_torch
    note_margin("reduce", f"power_blend backward {RC.NAME[arith]} P={power:.3g} device err / bound", worst, 1.0)
    note_margin("reduce", f"power_blend backward {RC.NAME[arith]} P={power:.3g} torch-cpu err / bound", worst_torch, 1.0)


# ---- 7. blend backward: zero semantics beyond fp64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [2.0, 0.5, 1.0])
@pytest.mark.parametrize("operand", [F32, torch.bfloat16, torch.float16], ids=RC.NAME.get)
def test_power_blend_backward_zero_semantics_fp32(operand, power, dev):
    "exact zeros in fp32 arithmetic: what torch autograd of the host expression gives in float32 (power 1 is the x^0 = 1 special case)"
    av, cv = (torch.tensor(col, dtype=operand) for col in RC.ZERO_TABLE)
    want = RC.blend_grads(av, cv, 0.5, 0.5, power, F32)
    got = _device_grads(av, cv, 0.5, 0.5, power, F32, dev)
    for side, (x, other) in enumerate(((av, cv), (cv, av))):
        g, w = got[side].cpu(), want[side]
        assert g.dtype == operand and torch.equal(torch.isnan(g), torch.isnan(w)), (power, side, g, w)
        ok = torch.isfinite(w).numpy()
        bound = RC.grad_bound(w.numpy(), x, 0.5, 0.5, other, power, operand, F32)
        assert (np.abs(g.double().numpy() - w.numpy())[ok] <= bound[ok]).all(), (power, side, g, w)
