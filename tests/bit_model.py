"""An exact host model of the step kernels' fp32 arithmetic (DESIGN.md sections 4.1, 4.5, 4.6, 4.7): individually rounded fp32 operations
in numpy, the contract of every step-family launch written with them, and a bit-for-bit comparison.

The contract, as the kernels' header comments state it: coefficients are narrowed to fp32 once; a sum starts from zero and takes one
fma per operand in slot order; the noise fma comes last (and is skipped, as a launch without noise, when zeta narrows to zero); the fp32
value is rounded once, to nearest even, to the output dtype.  A Runge-Kutta stage launch first evaluates out0 = from_x(s, to_x(s, o)) one
operation at a time -- multiply, subtract, divide, each rounded to fp32 and then to the tensor dtype (`convert`) -- and chains that
rounded derivative into out1 behind the operands and in front of the noise (`rk_stage`).

Exactness.  The product of two fp32 numbers has at most 48 significant bits and is exact in float64.  Adding a third fp32 number in
float64 rounds once; the TwoSum residual says in which direction, and moving an even float64 sum one place towards a non-zero residual
("round to odd") keeps that information in the last bit.  float64 carries 53 >= 2 * 24 + 2 bits, so rounding the odd-rounded sum to fp32
is the correctly rounded fp32 result -- overflow to inf and fp32 subnormals included.  The float64 quotient of two fp32 numbers, narrowed
once, is the correctly rounded fp32 quotient (`div32`).  inf, NaN and signed zeros go through float64's own IEEE rules.  tests/test_bit_model_host.py holds all of this against exact rational arithmetic.

Nothing here needs a GPU, and nothing is imported from conftest."""

from __future__ import annotations

import numpy as np
import torch


def widen(x) -> np.ndarray:
    "an operand as stored (torch tensor of bf16 / fp16 / fp32, or anything numpy takes) as the fp32 numbers a kernel widens it to: exact"
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().float().numpy()
    return np.asarray(x, dtype=np.float32)


def _wide(x) -> np.ndarray:
    with np.errstate(invalid="ignore"):  # (a signalling NaN pattern among the operands)
        return np.asarray(x, dtype=np.float32).astype(np.float64)


def _sum_to_odd(p: np.ndarray, c: np.ndarray) -> np.ndarray:
    "p + c in float64, rounded to odd: exact for the later rounding to fp32 whenever p and c are fp32 products or fp32 numbers"
    p, c = np.broadcast_arrays(np.atleast_1d(p), np.atleast_1d(c))
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # TwoSum: s + e == p + c exactly
        bits = s.view(np.int64)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((bits & 1) == 0)
        away = (e > 0) == (s > 0)  # the residual points away from zero (s == 0 with e != 0 cannot happen: a sum that cancels is exact)
        return np.where(fix, np.where(away, bits + 1, bits - 1), bits).view(np.float64)


def _narrow(s) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.asarray(s, dtype=np.float64).astype(np.float32)


def fma32(a, b, c) -> np.ndarray:
    "fl32(a * b + c): the correctly rounded fp32 fused multiply-add"
    with np.errstate(all="ignore"):
        return _narrow(_sum_to_odd(_wide(a) * _wide(b), _wide(c)))


def mul32(a, b) -> np.ndarray:
    "fl32(a * b): the product is exact in float64"
    with np.errstate(all="ignore"):
        return _narrow(_wide(a) * _wide(b))


def add32(a, b) -> np.ndarray:
    "fl32(a + b)"
    return _narrow(_sum_to_odd(_wide(a), _wide(b)))


def sub32(a, b) -> np.ndarray:
    "fl32(a - b)"
    return _narrow(_sum_to_odd(_wide(a), -_wide(b)))


def div32(a, b) -> np.ndarray:
    """fl32(a / b): the float64 quotient, narrowed once.  A quotient of two 24-bit numbers that is not itself a rounding boundary of fp32
    (a number of at most 25 bits; fewer in the subnormal range) lies further than 2^-(2 * 24 + 1) of its size from one, so the float64
    rounding (53 >= 2 * 24 + 2 bits) never moves it onto or across a boundary: the second rounding decides as one rounding would."""
    with np.errstate(all="ignore"):
        return _narrow(_wide(a) / _wide(b))


def round_to(dtype: torch.dtype, x32) -> torch.Tensor:
    """one RNE rounding of fp32 values to `dtype`: torch's CPU conversion of the fp32 tensor (held against an integer RNE on the bit
    patterns in tests/test_bit_model_host.py).  Never from float64: torch goes through fp32 there, which rounds twice."""
    x32 = np.ascontiguousarray(x32)
    assert x32.dtype == np.float32, x32.dtype
    return torch.from_numpy(x32.copy()).to(dtype)


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def _accumulate(coefs, xs, skip_zero: bool = False) -> np.ndarray:
    "s = 0; s = fma(c_k, x_k, s) in slot order, c_k narrowed to fp32; skip_zero: an operand whose narrowed coefficient is zero adds nothing"
    xs = [widen(x) for x in xs]
    assert len(coefs) == len(xs)
    s = np.zeros(xs[0].shape if xs else (), dtype=np.float32)
    for c, x in zip(coefs, xs):
        c32 = np.float32(c)
        if skip_zero and c32 == 0:
            continue
        s = fma32(c32, x, s)
    return s


def _noise(s, zeta, z):
    "the noise fma, last; none when there is no draw or zeta narrows to zero (the kernels' zero-zeta guard)"
    if zeta is None or z is None or np.float32(zeta) == 0:
        return s
    return fma32(np.float32(zeta), widen(z), s)


def step32(coef0, xs, zeta0=None, z0=None) -> np.ndarray:
    "the fp32 value of a one-output step before its rounding"
    return _noise(_accumulate(coef0, xs), zeta0, z0)


def step(coef0, xs, zeta0=None, z0=None, out: torch.dtype = torch.float32) -> torch.Tensor:
    "skr_step_launch, one output (skr_step.hip, skr_step_fast.hip)"
    return round_to(out, step32(coef0, xs, zeta0, z0))


def step_two(coef0, coef1, chain, xs, zeta0=None, z0=None, zeta1=None, z1=None, out0: torch.dtype = torch.float32, out1: torch.dtype = torch.float32):
    """skr_step_launch, two outputs: out0 as `step`, kept in fp32 for the chain; out1 accumulates coef1, then fma(chain, s0, s1), then its
    noise (the order tests/table_cases.py::emulate32 spells out for step_kernel_k2)"""
    s0 = step32(coef0, xs, zeta0, z0)
    s1 = _accumulate(coef1, xs)
    s1 = fma32(np.float32(chain), s0, s1)
    s1 = _noise(s1, zeta1, z1)
    return round_to(out0, s0), round_to(out1, s1)


def masked(coef0, coef1, xs, m, zeta0=None, z0=None, out: torch.dtype = torch.float32) -> torch.Tensor:
    "skr_step_launch_masked: s as `step`; k over the operands whose coef1 is not exactly zero; out = fma(m, s, mul(sub(1, m), k))"
    s = step32(coef0, xs, zeta0, z0)
    k = _accumulate(coef1, xs, skip_zero=True)
    m = widen(m)
    return round_to(out, fma32(m, s, mul32(sub32(np.float32(1), m), k)))


def backward(a, b, g0, g1=None, out: torch.dtype = torch.float32) -> torch.Tensor:
    "skr_step_backward_launch, one gradient: mul(a, g0), or fma(b, g1, mul(a, g0)) with two incoming gradients"
    o = mul32(np.float32(a), widen(g0))
    if g1 is not None:
        o = fma32(np.float32(b), widen(g1), o)
    return round_to(out, o)


def masked_backward(a, b, m, g, out: torch.dtype = torch.float32) -> torch.Tensor:
    "skr_step_masked_backward_launch, one gradient: t = sub(1, m); w = fma(a, m, mul(b, t)); o = mul(w, g)"
    m = widen(m)
    t = sub32(np.float32(1), m)
    w = fma32(np.float32(a), m, mul32(np.float32(b), t))
    return round_to(out, mul32(w, widen(g)))


# ---- Runge-Kutta stage launches (convert_rounded of skr_step_common.h; step_kernel_rk1, step_kernel_rk, step_kernel<..., CONV>) ------------
#   to_x   kinds: 0 o | 1 ((s - k0*o) / k1) | 2 (k1*s - k0*o) | 3 (o * k0)
#   from_x kinds: 0 x | 1 ((s - k2*x) / k3) | 2 ((k2*s - x) / k3) | 3 (x / k2)
def _convert(s, o, kinds, k, mul, sub, div, R):
    "from_x(s, to_x(s, o)) with every operation's result passed through R, in the order of the header's comment"
    to_kind, from_kind = kinds
    if to_kind == 1:
        x = R(div(R(sub(s, R(mul(k[0], o)))), k[1]))
    elif to_kind == 2:
        x = R(sub(R(mul(k[1], s)), R(mul(k[0], o))))
    elif to_kind == 3:
        x = R(mul(o, k[0]))
    else:
        x = o
    if from_kind == 1:
        return R(div(R(sub(s, R(mul(k[2], x)))), k[3]))
    if from_kind == 2:
        return R(div(R(sub(R(mul(k[2], s)), x)), k[3]))
    if from_kind == 3:
        return R(div(x, k[2]))
    return x


def convert32(dtype: torch.dtype, s, o, kinds, k, keep_last: bool = False) -> np.ndarray:
    """the stage's derivative as fp32 numbers that are values of `dtype`: k narrowed to fp32 once, every operation rounded to fp32 and
    then to `dtype`.  keep_last: the last operation's fp32 result without its rounding to `dtype` (what a wrong kernel might chain)"""
    k = [np.float32(v) for v in k]
    last = []

    def R(v):
        last[:] = [v]
        return widen(round_to(dtype, v))

    d = _convert(widen(s), widen(o), kinds, k, mul32, sub32, div32, R)
    return last[0] if keep_last and last else d


def convert(dtype: torch.dtype, s, o, kinds, k) -> torch.Tensor:
    """out0 of a stage launch: from_x(s, to_x(s, o)), one rounded operation at a time, a tensor of `dtype`.  torch.float64 (acc_f64
    launches over fp64 operands): the same operations in float64, k as the doubles they are, no second rounding."""
    if dtype == torch.float64:
        as64 = lambda t: t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)  # noqa: E731
        with np.errstate(all="ignore"):
            d = _convert(as64(s), as64(o), kinds, [np.float64(v) for v in k], np.multiply, np.subtract, np.divide, lambda v: v)
        return torch.from_numpy(np.ascontiguousarray(d).copy())
    return round_to(dtype, convert32(dtype, s, o, kinds, k))  # (exact: the values are values of `dtype`)


def rk_stage(coef1, chain, xs, kinds, k, zeta1=None, z1=None, out: torch.dtype | None = None):
    """skr_step_launch with a rounded conversion (fp32 arithmetic): out0 = convert(xs[0], xs[1]) in the pair's dtype; out1 accumulates
    coef1 over ALL operands from zero in slot order, then fma(chain, out0 widened to fp32, .) -- the derivative AFTER its rounding to the
    tensor dtype, in the general kernel's mixed launches too --, then the noise fma (none when zeta1 narrows to zero), then one
    rounding to `out` (the pair's dtype unless given).  Returns (out0, out1)."""
    dt = xs[0].dtype
    out0 = convert(dt, xs[0], xs[1], kinds, k)
    s1 = _accumulate(coef1, xs)
    s1 = fma32(np.float32(chain), widen(out0), s1)
    s1 = _noise(s1, zeta1, z1)
    return out0, round_to(out if out is not None else dt, s1)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------
_INT = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def bits_of(t: torch.Tensor) -> np.ndarray:
    "the integer view of a tensor's elements, flat, on the host"
    return t.detach().cpu().contiguous().view(_INT[t.dtype]).numpy().reshape(-1)


def differing(got: torch.Tensor, want: torch.Tensor) -> np.ndarray:
    "flat bool array: where `got` has other bits than `want` (a NaN equals any NaN; -0 and +0 differ)"
    assert got.dtype == want.dtype and got.numel() == want.numel(), (got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    gn, wn = torch.isnan(g).numpy(), torch.isnan(w).numpy()
    return np.where(gn | wn, gn != wn, bits_of(g) != bits_of(w))


def same_bits(got: torch.Tensor, want: torch.Tensor, operands=(), what: str = "") -> None:
    """Every element of `got` has the bits of `want`: NaN exactly where `want` has NaN, the same integer view everywhere else.  A failure
    says how many differ and shows the first few: index, the bits got and wanted, the bits of `operands` there."""
    bad = differing(got, want)
    if not bad.any():
        return
    gb, wb = bits_of(got), bits_of(want)
    width = 4 if got.dtype in (torch.bfloat16, torch.float16) else 8
    lines = []
    for i in np.flatnonzero(bad)[:6]:
        ops = " ".join(f"{int(bits_of(o)[i]) & (2 ** (8 * o.element_size()) - 1):0{2 * o.element_size()}x}" for o in operands if o.numel() == got.numel())
        lines.append(f"  [{int(i)}] got {int(gb[i]) & (16 ** width - 1):0{width}x} want {int(wb[i]) & (16 ** width - 1):0{width}x} operands {ops}")
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits\n" + "\n".join(lines))
