"""Inputs, high-precision references and DERIVED bars shared by test_reduce_gpu.py and test_reduce_host.py: the error norm
(skr_error_mean / lazy.error_mean) and the signed-power blend with its backward (skr_power_blend[_backward] / lazy.power_blend).

Nothing here is measured on the code under test.  The norm's bar counts the additions on the longest path of the kernel's
fixed-order double-precision sum; the blend's is the elementwise error model of test_round3_gpu.py (K = 64), in eps32 for an fp32
result and in eps64 for an fp64 one; the backward's propagates the same inner-sum error through the derivative of the outer power."""

import math
from fractions import Fraction

import numpy as np
import torch
from test_round3_gpu import _spow  # the reference's definition, sign(0) = +1 (common.py:187-190)

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]
NAME = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32", torch.float64: "f64"}
MANTISSA = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24, torch.float64: 53}  # significand bits, hidden one included
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126, torch.float64: -1022}
EPS = {torch.float32: 2.0**-23, torch.float64: 2.0**-52}
K = 64.0
WEIGHTS = [(0.35, 0.65), (1.7, -0.7)]  # (a negative weight: cancellation between same-signed operands)

# ---- error norm ----------------------------------------------------------------------------------------------------------------
NORM_BLOCKS, NORM_LANES = 1024, 256  # the kernel's grid cap and workgroup size: the stride loop runs above 262144 elements
NORM_SIZES = [1, 63, 64, 65, 255, 256, 257, 3000, 262143, 262144, 262145, 2 * 262144 + 777]
NORM_EXACT_SIZES = NORM_SIZES[:3]  # also evaluated in rational arithmetic


def norm_inputs(numel: int, dtype: torch.dtype, seed: int):
    """randn times a slow ramp 1 + i / numel, rounded once to `dtype`: an element that is dropped, repeated or taken from a shifted
    position moves the mean by ~1 / numel of itself, 1e-6 at the largest size, seven orders above the bar"""
    g = torch.Generator().manual_seed(seed)
    ramp = 1.0 + torch.arange(numel, dtype=torch.float64) / numel
    a = (torch.randn(numel, generator=g, dtype=torch.float64) * ramp).to(dtype)
    b = (torch.randn(numel, generator=g, dtype=torch.float64) * ramp).to(dtype)
    return a, b


def _summands(a, b, power: int) -> np.ndarray:
    "the kernel's summands in its own arithmetic: the widening is exact, the subtraction and the square are one double rounding each"
    bw = b.double().numpy().ravel()
    d = np.abs((a.double().numpy().ravel() if a is not None else 0.0) - bw)
    return d * d if power == 2 else d


def norm_exact(a, b, power: int) -> float:
    "exactly rounded sum (math.fsum) of the float64 summands, over numel"
    s = _summands(a, b, power)
    return math.fsum(s.tolist()) / s.size


def norm_fraction(a, b, power: int) -> Fraction:
    "mean(|a - b|^power) of the dtype-rounded inputs in rational arithmetic: no rounding anywhere"
    bw = [Fraction(v) for v in b.double().ravel().tolist()]
    aw = [Fraction(v) for v in a.double().ravel().tolist()] if a is not None else [Fraction(0)] * len(bw)
    return sum((abs(x - y) ** power for x, y in zip(aw, bw)), Fraction(0)) / len(bw)


def norm_bar(numel: int) -> float:
    """Relative bar.  Every summand is >= 0, so a fixed-order double-precision sum is off by at most (additions on the longest
    path) * 2^-53 relative: T trips of the stride loop, six shuffle steps, three LDS adds, B additions of the final loop, and one
    rounding each for the subtraction, the square and the division."""
    blocks = min(NORM_BLOCKS, -(-numel // NORM_LANES))
    trips = -(-numel // (NORM_LANES * blocks))
    return 1.01 * (trips + 6 + 3 + blocks + 3) * 2.0**-53


def subnormals(dtype: torch.dtype) -> torch.Tensor:
    "every positive subnormal of a 16-bit dtype (1000 of them for fp32), from their bit patterns"
    if dtype == torch.float32:
        return torch.arange(1, 1001, dtype=torch.int32).view(torch.float32)
    return torch.arange(1, 1 << (MANTISSA[dtype] - 1), dtype=torch.int16).view(dtype)


# ---- signed-power blend, forward ---------------------------------------------------------------------------------------------
BLEND_N = 3 * 256 + 37
BLEND_POWERS = [0.5, 2.0, 3.0, 1.0 / 3.0, 0.75]
BLEND_STRIDE_BLOCKS = 8192  # grid cap: the stride loop runs above 8192 * 256 elements


def blend_inputs(n: int, seed: int, power: float, wp: float, wc: float, cancel: bool, a_dtype, c_dtype):
    """randn operands rounded to their dtypes; with `cancel`, the constructed cancellation of test_power_blend_error_model: in the
    first quarter the two powered terms nearly annihilate (to 1e-4, or to the rounding of a narrower dtype)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=g, dtype=torch.float64).to(a_dtype)
    c = torch.randn(n, generator=g, dtype=torch.float64)
    if cancel:
        q = a[: n // 4].double()
        t = (abs(wp) * q.abs().pow(power) / abs(wc)).pow(1.0 / power) * (1 + 1e-4 * torch.randn(n // 4, generator=g, dtype=torch.float64))
        c[: n // 4] = t * torch.where((q < 0) ^ (wp * wc > 0), 1.0, -1.0)
    return a, c.to(c_dtype)


def _spow_np(v, f):
    "_spow on numpy arrays (float64 or longdouble): |v|^f * (-1 if v < 0 else +1)"
    return np.abs(v) ** f * np.where(v < 0, -1.0, 1.0).astype(v.dtype)


def wide_of(result_dtype):
    "the precision the reference is evaluated in: float64 for an fp32 result, the 64-bit-mantissa long double for an fp64 one"
    if result_dtype == torch.float32:
        return np.float64
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is no wider than float64 on this platform"
    return np.longdouble


def widen(t: torch.Tensor, wide) -> np.ndarray:
    return t.detach().cpu().double().numpy().astype(wide)


class BlendRef:
    "exact value, inner sum u, S = |wp||a|^P + |wc||c|^P and scale = S^(1/P) of one blend, on the dtype-rounded operands"

    def __init__(self, a, c, wp, wc, power, result_dtype):
        wide = wide_of(result_dtype)
        self.power, self.eps, self.wide = power, EPS[result_dtype], wide
        aw, cw, P, inv = widen(a, wide), widen(c, wide), wide(power), wide(1.0 / power)
        with np.errstate(all="ignore"):
            self.u = wide(wp) * _spow_np(aw, P) + wide(wc) * _spow_np(cw, P)
            self.exact = _spow_np(self.u, inv)
            self.S = abs(wide(wp)) * np.abs(aw) ** P + abs(wide(wc)) * np.abs(cw) ** P
            self.scale = self.S**inv

    def bound(self) -> np.ndarray:
        """|got - exact| <= 1e-5 max|exact| + K eps32 scale (test_round3_gpu.py), every eps32 an eps of the result arithmetic
        (1e-5 is 83.9 eps32).  For P > 1 the outer power is unbounded at u = 0 and the inner error K eps S is carried through it."""
        eps, inv = self.eps, self.wide(1.0 / self.power)
        finite = np.isfinite(self.exact)
        floor = (1e-5 * eps / EPS[torch.float32]) * (np.abs(self.exact[finite]).max() if finite.any() else 0.0)
        with np.errstate(all="ignore"):
            bound = K * eps * self.scale
            if self.power > 1:
                du = K * eps * self.S
                bound = np.maximum((np.abs(self.u) + du) ** inv - np.maximum(np.abs(self.u) - du, 0) ** inv, bound)
        return floor + bound

    def margin(self, got: torch.Tensor) -> float:
        "worst err / bound over the finite entries (< 1 passes)"
        with np.errstate(all="ignore"):
            err, bound = np.abs(widen(got, self.wide) - self.exact), self.bound()
        ok = np.isfinite(self.exact)
        assert np.isfinite(err[ok]).all(), "a non-finite result where the exact value is finite"
        with np.errstate(all="ignore"):
            ratio = np.where(err[ok] == 0, 0.0, err[ok] / bound[ok])
        return float(ratio.max()) if ok.any() else 0.0

    def units(self, got: torch.Tensor) -> float:
        """worst error in units of eps * scale, with no floor term (the wide-range measurement).  For P > 1, where the outer power
        amplifies without bound near u = 0, an element is also measured through u, |spow(got, P) - u| / (eps S), and counts with
        the smaller figure -- the two branches of bound()."""
        g = widen(got, self.wide)
        with np.errstate(all="ignore"):
            k = np.abs(g - self.exact) / (self.eps * self.scale)
            if self.power > 1:
                k = np.minimum(k, np.abs(_spow_np(g, self.wide(self.power)) - self.u) / (self.eps * self.S))
        return float(k.max())


def blend_torch(a, c, wp, wc, power, result_dtype) -> torch.Tensor:
    "the reference formula in the result arithmetic on the CPU (torch)"
    a, c = a.detach().cpu().to(result_dtype), c.detach().cpu().to(result_dtype)
    return _spow(wp * _spow(a, power) + wc * _spow(c, power), 1.0 / power)


SPECIALS = [0.0, -0.0, 1.5, -1.5, math.inf, -math.inf, math.nan]


def special_pairs(dtype=torch.float64):
    "all pairs of {+0, -0, +-1.5, +-inf, NaN}; (1.5, -1.5) and (-1.5, 1.5) cancel exactly under equal weights"
    a = torch.tensor([x for x in SPECIALS for _ in SPECIALS], dtype=dtype)
    c = torch.tensor([y for _ in SPECIALS for y in SPECIALS], dtype=dtype)
    return a, c


def assert_same_specials(got: torch.Tensor, want: torch.Tensor, what) -> None:
    "same NaN pattern, same infinities with sign, same sign of every zero"
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN pattern", got, want)
    assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want)), (what, "inf pattern", got, want)
    zero = want == 0
    assert torch.equal(got == 0, zero), (what, "zeros", got, want)
    assert torch.equal(torch.signbit(got[zero]), torch.signbit(want[zero])), (what, "sign of zero", got, want)


# ---- signed-power blend, backward --------------------------------------------------------------------------------------------
GRAD_POWERS = [2.0, 0.5, 3.0]
ZERO_TABLE = ([0.0, 1.5, 0.0, -2.0], [0.0, 0.0, 2.0, 2.0])  # the table of test_gradcheck_power_blend_and_zero_semantics


def blend_grads(a, c, wp, wc, power, arith) -> tuple:
    "torch autograd of the reference expression on CPU copies of the operands, evaluated in `arith`; (grad a, grad c) as float64"
    al, cl = a.detach().cpu().to(arith).requires_grad_(), c.detach().cpu().to(arith).requires_grad_()
    _spow(wp * _spow(al, power) + wc * _spow(cl, power), 1.0 / power).sum().backward()
    return al.grad.double(), cl.grad.double()


def half_ulp(exact: np.ndarray, grad_dtype, arith) -> np.ndarray:
    "half an ULP of the gradient's dtype at `exact`; nothing where the store does not round (the gradient is as wide as the arithmetic)"
    if MANTISSA[grad_dtype] >= MANTISSA[arith]:
        return np.zeros_like(exact)
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.abs(exact)))
    e = np.maximum(np.where(np.isfinite(e), e, MIN_EXP[grad_dtype]), MIN_EXP[grad_dtype])
    return np.exp2(e - (MANTISSA[grad_dtype] - 1) - 1)


def grad_bound(exact, x, w, c_other, x_other, power, grad_dtype, arith) -> np.ndarray:
    """|got - exact| <= half_ulp + K eps (|exact| + cancellation scale), per element, for the gradient w.r.t. operand x of weight w.

    grad = g w P |x|^(P-1) h(|u|), h(m) = (1/P) m^(1/P - 1), u = w spow(x, P) + c_other spow(x_other, P).  The arithmetic computes u
    with |du| <= K eps S (the forward model), so h is off by at most max |h(|u| +- du) - h(|u|)| (h is monotone; |u| - du is clamped
    at 0, where h is infinite for P > 1: no bound exists where the inner sum cancels to its own rounding).  To first order that is
    K eps |exact| |1/P - 1| S / |u|."""
    eps, inv = EPS[arith], 1.0 / power
    xw, ow = x.detach().cpu().double().numpy(), x_other.detach().cpu().double().numpy()
    with np.errstate(all="ignore"):
        u = np.abs(w * _spow_np(xw, power) + c_other * _spow_np(ow, power))
        du = K * eps * (abs(w) * np.abs(xw) ** power + abs(c_other) * np.abs(ow) ** power)
        h = lambda m: inv * m ** (inv - 1.0)  # noqa: E731
        dh = np.maximum(np.abs(h(u + du) - h(u)), np.abs(h(np.maximum(u - du, 0.0)) - h(u)))
        carried = abs(w) * power * np.abs(xw) ** (power - 1.0) * dh
    carried = np.where(np.isnan(carried), np.inf, carried)
    return half_ulp(exact, grad_dtype, arith) + K * eps * np.abs(exact) + carried
