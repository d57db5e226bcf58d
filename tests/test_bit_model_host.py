"""The exact model of the step kernels' fp32 arithmetic (tests/bit_model.py) and its inputs (tests/bit_cases.py), checked on the host:

  * the model is right: fma32 against exact rational arithmetic, round_to against an integer round-to-nearest-even on the bit patterns;
  * the inputs are sharp: TIES and PATTERNS hold the classes of elements at which a wrong kernel gives other bits, counted from the model;
  * the tests can fail: six wrong variants of the contract, built on the host only, each differ from the model on many elements;
  * the Runge-Kutta stage family: div32 against exact rational arithmetic, convert against CPU torch op by op on every conversion input,
    and four wrong conversions and five wrong stages counted against the model.

tests/test_bit_contract_gpu.py holds the kernels to the model with these inputs."""

from fractions import Fraction

import bit_cases as BC
import bit_model as BM
import numpy as np
import pytest
import table_cases as TC
import torch
from skr_oracle import noise as ON


# ---- exact references -------------------------------------------------------------------------------------------------------------------
def fl32_of_fraction(x: Fraction, zero_sign: int) -> int:
    "the fp32 bit pattern of the exact rational x rounded to nearest even: overflow to inf, gradual underflow; zero_sign: the sign bit of an exact zero"
    if x == 0:
        return zero_sign << 31
    sign, x = (1 if x < 0 else 0), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if x < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    e = max(e, -126)
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    if n == 2**24:
        n, e = 2**23, e + 1
    if e > 127:
        return (sign << 31) | 0x7F800000
    if n < 2**23:  # subnormal (or zero): e == -126
        return (sign << 31) | n
    return (sign << 31) | ((e + 127) << 23) | (n - 2**23)


def exact_fma_bits(a: np.float32, b: np.float32, c: np.float32) -> int:
    fa, fb, fc = float(a), float(b), float(c)
    ps = int(np.signbit(a)) ^ int(np.signbit(b))
    zero_sign = ps if (fa == 0 or fb == 0) and fc == 0 and ps == int(np.signbit(c)) else 0  # (-0) + (-0) = -0; every other exact zero is +0
    return fl32_of_fraction(Fraction(fa) * Fraction(fb) + Fraction(fc), zero_sign)


def finite_patterns(rng, n: int) -> np.ndarray:
    x = rng.integers(0, 2**32, 2 * n + 64, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return x[np.isfinite(x)][:n]


def scaled(rng, n: int, lo: int, hi: int) -> np.ndarray:
    "random significands at exponents lo .. hi, both signs"
    return (np.ldexp(rng.uniform(1, 2, n), rng.integers(lo, hi + 1, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def fma_triples():
    rng = np.random.default_rng(2024)
    sets = []
    a, b, c = finite_patterns(rng, 3000), finite_patterns(rng, 3000), finite_patterns(rng, 3000)
    sets.append((a, b, c))  # random bit patterns (zeros and subnormals included)
    a, b = scaled(rng, 1500, -20, 20), scaled(rng, 1500, -20, 20)
    with np.errstate(all="ignore"):
        c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)  # cancellation: c = -fl32(a b) and its two neighbours
    sets += [(a, b, c), (a, b, np.nextafter(c, np.float32(np.inf))), (a, b, np.nextafter(c, np.float32(-np.inf)))]
    a, b = scaled(rng, 1500, 62, 64), scaled(rng, 1500, 62, 64)  # products around 2^127: the overflow threshold
    sets.append((a, b, scaled(rng, 1500, 100, 127)))
    a, b = scaled(rng, 1500, -80, -68), scaled(rng, 1500, -80, -68)  # products in and below the subnormal range
    c = np.where(rng.random(1500) < 0.5, rng.integers(0, 2**23, 1500).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    sets.append((a, b, c * rng.choice([-1.0, 1.0], 1500).astype(np.float32)))
    # crafted: max + half an ulp is the tie that rounds to inf, just below it stays max; the smallest subnormal's half; signed zeros
    big, top = np.float32(2.0**64), np.float32((2 - 2.0**-23) * 2.0**63)
    half = np.float32(2.0**103)
    tiny = np.float32(2.0**-75)
    craft = [(big, top, half), (big, top, np.nextafter(half, np.float32(0))), (-big, top, -half), (big, top, -half),
             (tiny, tiny, np.float32(0)), (tiny, np.nextafter(tiny, np.float32(1)), np.float32(0)), (tiny, tiny, np.float32(2.0**-149)),
             (np.float32(1), np.float32(-0.0), np.float32(0.0)), (np.float32(1), np.float32(-0.0), np.float32(-0.0)), (np.float32(-1), np.float32(0.0), np.float32(0.0)),
             (np.float32(3), np.float32(2), np.float32(-6))]  # fmt: skip
    sets.append(tuple(np.array(col, dtype=np.float32) for col in zip(*craft)))
    return sets


def test_fma32_is_the_correctly_rounded_fused_multiply_add():
    checked = 0
    for a, b, c in fma_triples():
        got = BM.fma32(a, b, c).view(np.uint32)
        for i in range(a.size):
            want = exact_fma_bits(a[i], b[i], c[i])
            assert int(got[i]) == want, (a[i], b[i], c[i], hex(int(got[i])), hex(want))
        checked += a.size
    assert checked >= 10000, checked


def test_mul32_add32_sub32_are_correctly_rounded():
    rng = np.random.default_rng(7)
    a, b = finite_patterns(rng, 1500), finite_patterns(rng, 1500)
    s, t = scaled(rng, 1500, -3, 3), scaled(rng, 1500, -30, 3)
    one, zero = np.float32(1), np.float32(0)
    mul, add, sub = BM.mul32(a, b).view(np.uint32), BM.add32(s, t).view(np.uint32), BM.sub32(s, t).view(np.uint32)
    raw = BM.add32(a, b).view(np.uint32)
    for i in range(1500):
        assert int(mul[i]) == exact_fma_bits(a[i], b[i], np.float32(-0.0) if np.signbit(a[i]) != np.signbit(b[i]) else zero), (a[i], b[i])
        assert int(add[i]) == exact_fma_bits(s[i], one, t[i]) and int(sub[i]) == exact_fma_bits(s[i], one, -t[i]), (s[i], t[i])
        assert int(raw[i]) == exact_fma_bits(a[i], one, b[i]), (a[i], b[i])


def rne_bf16_bits(b: np.ndarray) -> np.ndarray:
    "fp32 bit patterns -> bf16 bit patterns, round to nearest even, written on the integers (NaN: 0x7FC0)"
    b = b.astype(np.int64)
    nan = ((b >> 23) & 0xFF == 255) & (b & 0x7FFFFF != 0)
    return np.where(nan, 0x7FC0, (b + 0x7FFF + ((b >> 16) & 1)) >> 16)


def rne_f16_bits(b: np.ndarray) -> np.ndarray:
    "fp32 bit patterns -> fp16 bit patterns, round to nearest even, written on the integers (NaN: 0x7E00)"
    b = b.astype(np.int64)
    sign, e, m = (b >> 16) & 0x8000, (b >> 23) & 0xFF, b & 0x7FFFFF
    nan = (e == 255) & (m != 0)
    sig, ee = np.where(e > 0, m | 0x800000, m), np.where(e > 0, e, 1)  # the value is sig * 2^(ee - 150)
    big_e = ee - 127
    shift = np.minimum(np.where(big_e >= -14, 13, 13 + (-14 - big_e)), 40)  # bits below the fp16 unit: normal, or the subnormal unit 2^-24
    q, rem, halfway = sig >> shift, sig & ((np.int64(1) << shift) - 1), np.int64(1) << (shift - 1)
    q = q + ((rem > halfway) | ((rem == halfway) & (q & 1 == 1)))
    out = np.where(big_e >= -14, ((big_e + 15) << 10) + q - 1024, q)  # (a carry out of the significand walks into the exponent)
    out = np.minimum(out, 0x7C00) | sign
    return np.where(nan, 0x7E00, out)


@pytest.mark.parametrize("name", BC.NARROW)
def test_round_to_is_one_rne_rounding_at_every_boundary(name):
    "the midpoint behind every pattern of the dtype and its two fp32 neighbours: 3 x 65 536 values"
    dt = BC.DTYPES[name]
    pats = BC.patterns(name)
    a = pats.float()
    nxt = (pats.view(torch.int16) + 1).view(dt).float()
    mid = ((a.double() + nxt.double()) / 2).float()  # exact: one more bit than the dtype
    ok = torch.isfinite(a) & torch.isfinite(nxt) & torch.isfinite(mid)
    top = torch.isfinite(a) & torch.isinf(nxt)  # the overflow threshold: max + half its unit, written out
    unit = (a - (pats.view(torch.int16) - 1).view(dt).float()).double()
    mid = torch.where(top, (a.double() + unit / 2).float(), torch.where(ok, mid, a))
    mid_bits = mid.numpy().view(np.int32).astype(np.int64)
    rne = rne_bf16_bits if name == "bf16" else rne_f16_bits
    sticky_ties = 0
    for d in (-1, 0, 1):
        bits = (mid_bits + d).astype(np.uint32)  # (NaN patterns stay NaN, the infs step to max and to a NaN)
        x = bits.view(np.float32)
        got = BM.round_to(dt, x)
        want = rne(bits)
        isnan = np.isnan(x)
        assert np.array_equal(torch.isnan(got).numpy(), isnan)
        got_bits = got.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
        assert np.array_equal(got_bits[~isnan], want[~isnan]), (name, d, int((got_bits[~isnan] != want[~isnan]).sum()))
        if d == 0:
            exact = ~isnan & (ok | top).numpy()
            with np.errstate(invalid="ignore"):  # (the NaN patterns)
                up = BM.round_to(dt, np.nextafter(x, np.float32(np.inf))).view(torch.int16).numpy()
                down = BM.round_to(dt, np.nextafter(x, np.float32(-np.inf))).view(torch.int16).numpy()
            sticky_ties = int((up != down)[exact].sum())
    assert sticky_ties >= 65000 if name == "bf16" else sticky_ties >= 63000, sticky_ties  # (the midpoints really are ties)


# ---- one rounding of an exact value: what a fused multiply-add-and-convert stores --------------------------------------------------------
PRECISION = {torch.bfloat16: (8, -126), torch.float16: (11, -14), torch.float32: (24, -126)}


def round_once(dt: torch.dtype, x64: np.ndarray) -> torch.Tensor:
    """RNE of float64 values straight to `dt`: scale by the dtype's unit at that magnitude (a power of two, exact), np.rint (halves to
    even), scale back -- the result is a value of the dtype, so the two conversions behind it are exact.  x64: exact, or rounded to odd."""
    p, emin = PRECISION[dt]
    with np.errstate(all="ignore"):
        _, e = np.frexp(x64)  # |x| in [2^(e-1), 2^e)
        unit = np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
        r = np.where(np.isfinite(x64), np.rint(x64 / unit) * unit, x64)
        return torch.from_numpy(r.astype(np.float32)).to(dt)


def test_round_once_agrees_with_the_model_on_fp32_inputs():
    rng = np.random.default_rng(3)
    x = np.concatenate([finite_patterns(rng, 20000), scaled(rng, 20000, -30, 17), scaled(rng, 5000, -140, -120)])
    for dt in (torch.bfloat16, torch.float16):
        BM.same_bits(round_once(dt, x.astype(np.float64)), BM.round_to(dt, x), what=f"round_once {dt}")


# ---- the contract and its wrong variants ------------------------------------------------------------------------------------------------
def mul_add(a, b, c):
    return BM.add32(BM.mul32(a, b), c)


def flush32(x, dt):
    """fp32 subnormals to zero (sign kept); for a tensor stored as fp16 also what is subnormal there: its conversions from and to fp32 are
    what a flushing mode changes for it (an fp16 subnormal is a normal fp32 number)"""
    x = np.asarray(x, dtype=np.float32)
    tiny = np.float32(2.0**-14 if dt == torch.float16 else 2.0**-126)
    return np.where(np.abs(x) < tiny, np.copysign(np.float32(0), x), x).astype(np.float32)


def evaluate(coefs, xs, dt, zeta=None, z=None, variant=None) -> torch.Tensor:
    "a one-output step into dtype `dt` by the contract (variant None: bit_model.step) or by one of the wrong variants"
    if variant is None:
        return BM.step(coefs, xs, zeta, z, out=dt)
    stored = [x.dtype if isinstance(x, torch.Tensor) else torch.float32 for x in xs]
    xs = [BM.widen(x) for x in xs]
    if variant == "flushed":
        xs = [flush32(x, sd) for x, sd in zip(xs, stored)]
    terms = [(np.float32(c), x) for c, x in zip(coefs, xs)]
    noise = [(np.float32(zeta), BM.widen(z))] if zeta is not None and np.float32(zeta) != 0 else []
    fma = BM.fma32
    if variant == "mul_add":
        fma = mul_add
    if variant == "reversed":
        terms = terms[::-1]
    terms = noise + terms if variant == "noise_first" else terms + noise
    if variant == "flushed":
        fma = lambda a, b, c: flush32(BM.fma32(a, b, c), torch.float32)  # noqa: E731
    s = np.zeros(xs[0].shape, dtype=np.float32)
    for c, x in terms[:-1]:
        s = fma(c, x, s)
    c, x = terms[-1]
    if variant == "fused":  # the last fma and the conversion as one instruction: the exact sum, rounded once
        with np.errstate(all="ignore"):
            return round_once(dt, BM._sum_to_odd(BM._wide(c) * BM._wide(x), BM._wide(s)))
    s = fma(c, x, s)
    out = BM.round_to(dt, s)
    if variant == "flushed":
        out = torch.from_numpy(flush32(out.float().numpy(), dt)).to(dt)
    return out


RANDOM_KS = (2, 5, 9, 17)
ZETA, STREAM, SEED = TC.ZETAS[0], TC.STREAMS[0], TC.SEEDS[0]


def host_normal(n: int) -> np.ndarray:
    return np.concatenate([ON.philox_normal(SEED + b, STREAM, BC.SAMPLE) for b in range(n // BC.SAMPLE)]).astype(np.float32)


def variant_differences(name: str, variant: str) -> dict:
    """Elements of TIES u RANDOM (fp32: RANDOM u SPECIALS) where the variant has other bits than the contract, by where they are found,
    over the outputs tests/test_bit_contract_gpu.py compares for these operands: the output in the operands' dtype and, for 16-bit
    operands, the fp32 output and the cancelling sum of the mixed-group launches.  A last-place difference of the fp32 value survives
    the rounding to a 16-bit output of unrelated normals once in 2^15, so a wrong order or a split fma shows in the 16-bit output of
    RANDOM in a few elements only -- enough to fail a comparison without tolerance, too few to count on; the other two outputs are
    where it shows in bulk."""
    dt = BC.DTYPES[name]
    noisy = variant == "noise_first"
    z = host_normal(BC.SAMPLES * BC.SAMPLE) if noisy else None
    zeta = ZETA if noisy else None

    def count(coefs, ops, out, zeta=None, z=None):
        return int(BM.differing(evaluate(coefs, ops, out, zeta, z, variant=variant), evaluate(coefs, ops, out, zeta, z)).sum())

    n = {}
    if name in BC.NARROW and not noisy:
        n["ties"] = sum(count(BC.tie_coefs(k3), BC.tie_operands(name), dt) for k3 in BC.TIE_K3)
    if name == "fp32" and not noisy:
        n["specials"] = count(BC.SPECIAL_COEFS, BC.specials32(), dt)
    n["random"] = sum(count(BC.random_coefs(k, "step"), BC.random_operands(name, k), dt, zeta, z) for k in RANDOM_KS)
    if name in BC.NARROW:
        if variant != "fused":  # (one rounding of the exact sum IS the fma of an fp32 output)
            n["random_fp32_out"] = count(BC.random_coefs(5, "step"), BC.random_operands(name, 5), torch.float32, zeta, z)
        mixed = [BC.mixed_operands(name, k, zeta, z) for k in BC.MIXED_KS]
        n["mixed_cancelling"] = sum(count(coefs, ops, dt, zeta, z) for ops, coefs in mixed)
    return n


@pytest.mark.parametrize("variant", ["fused", "mul_add", "reversed", "noise_first", "flushed"])
@pytest.mark.parametrize("name", BC.NARROW)
def test_a_wrong_step_differs_from_the_contract_16_bit(name, variant):
    n = variant_differences(name, variant)
    print(f"{name} {variant}: {sum(n.values())} elements differ {n}")
    assert sum(n.values()) >= 1000, (name, variant, n)
    assert n["random"] + n.get("ties", 0) + n["mixed_cancelling"] >= 1000, (name, variant, n)  # (in 16-bit outputs alone)


@pytest.mark.parametrize("variant", ["mul_add", "reversed", "noise_first", "flushed"])
def test_a_wrong_step_differs_from_the_contract_fp32(variant):
    "(a fused multiply-add-and-convert does not exist for an fp32 output: one rounding of the exact sum IS the fma)"
    n = variant_differences("fp32", variant)
    print(f"fp32 {variant}: {sum(n.values())} elements differ {n}")
    assert sum(n.values()) >= 100, (variant, n)


def soft_mask_flat(dt: torch.dtype, eighth: bool = False) -> torch.Tensor:
    mask_numel = BC.SAMPLE // 8 if eighth else BC.SAMPLE
    return BC.expand_mask(BC.soft_mask(dt, BC.SAMPLES, mask_numel, 5), mask_numel, BC.SAMPLES, BC.SAMPLE)


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_a_blend_of_two_products_and_an_add_differs_from_the_masked_contract(name):
    """RANDOM under the soft masks; for the 16-bit dtypes also the cancelling blend of the general kernel's mixed-group launch (see
    variant_differences: among unrelated normals a 16-bit output hides all but a few last-place differences of the fp32 value)"""
    dt = BC.DTYPES[name]
    m = soft_mask_flat(dt)
    cases = [(BC.random_operands(name, k), BC.random_coefs(k, "masked0"), BC.masked_coef1(k)) for k in (2, 5, 9)]
    if name in BC.NARROW:
        cases += [BC.masked_cancelling(name, k, m) for k in BC.MIXED_KS]
    n = []
    for ops, c0, c1 in cases:
        want = BM.masked(c0, c1, ops, m, out=dt)
        s, kn, m32 = BM.step32(c0, ops), BM._accumulate(c1, ops, skip_zero=True), BM.widen(m)
        wrong = BM.round_to(dt, BM.add32(BM.mul32(m32, s), BM.mul32(BM.sub32(np.float32(1), m32), kn)))
        n.append(int(BM.differing(wrong, want).sum()))
    print(f"{name} two products and an add: {sum(n)} elements differ {n}")
    assert sum(n) >= (100 if name == "fp32" else 1000), (name, n)


# ---- the inputs are sharp ---------------------------------------------------------------------------------------------------------------
def tie_classes(name: str) -> dict:
    "what TIES holds, from the model alone: per class the number of elements in front of the padding, summed over the five k3"
    dt = BC.DTYPES[name]
    _, _, kept = BC.ties(name)
    out = {"kept": kept, "fused_differs": 0, "exact_ties": 0, "value_on_tie_inexact": 0, "subnormal_results": 0, "inf_pos": 0, "inf_neg": 0}
    tiny = float(torch.finfo(dt).tiny)
    for k3 in BC.TIE_K3:
        ops, coefs = BC.tie_operands(name), BC.tie_coefs(k3)
        s = BM.step32(coefs, ops)[:kept]
        two = BM.round_to(dt, s)
        on_tie = (BM.differing(BM.round_to(dt, np.nextafter(s, np.float32(np.inf))), BM.round_to(dt, np.nextafter(s, np.float32(-np.inf)))) &
                  (two.float().numpy() != s))  # fmt: skip
        if k3 == 0.0:
            out["exact_ties"] += int(on_tie.sum())
            r = two.float().numpy()
            out["subnormal_results"] += int(((np.abs(r) < tiny) & (r != 0)).sum())
            out["inf_pos"] += int((r == np.inf).sum())
            out["inf_neg"] += int((r == -np.inf).sum())
        if abs(k3) == 2.0**-18:
            out["value_on_tie_inexact"] += int(on_tie.sum())
        out["fused_differs"] += int(BM.differing(evaluate(coefs, ops, dt, variant="fused"), evaluate(coefs, ops, dt))[:kept].sum())
    return out


@pytest.mark.parametrize("name", BC.NARROW)
def test_ties_hold_the_elements_a_wrong_rounding_cannot_pass(name):
    got = tie_classes(name)
    print(name, got)
    assert got["fused_differs"] >= 30000 and got["exact_ties"] >= 60000, got
    assert got["subnormal_results"] >= (2000 if name == "fp16" else 250), got
    assert got["inf_pos"] >= 1 and got["inf_neg"] >= 1, got
    a, u, kept = BC.ties(name)
    assert a.numel() % BC.CHUNK == 0 and a.numel() <= 65536 and (a[kept:].float() == 1).all() and (u[kept:].float() == 1).all()


@pytest.mark.parametrize("name", BC.NARROW)
def test_patterns_hold_every_nan_and_every_subnormal(name):
    p = BC.patterns(name)
    f = p.float()
    assert p.numel() == 65536 and np.array_equal(np.sort(BM.bits_of(p).astype(np.int64) & 0xFFFF), np.arange(65536))
    mant = 10 if name == "fp16" else 7
    assert int(torch.isnan(f).sum()) == 2 * (2**mant - 1) and int(torch.isinf(f).sum()) == 2
    assert int(((f.abs() < float(torch.finfo(BC.DTYPES[name]).tiny)) & (f != 0)).sum()) == 2 * (2**mant - 1)
    assert int((f == 0).sum()) == 2 and int(torch.signbit(f[f == 0]).sum()) == 1
    # fma(1, -0, +0) is +0: the model, not the identity, is the reference of the PATTERNS launches
    want = BM.step([1.0], [p], out=BC.DTYPES[name])
    assert int(BM.differing(want, p).sum()) == 1 and BM.bits_of(want)[0x8000] == 0


def test_specials_hold_what_the_issue_lists():
    x0, _ = BC.specials32()
    x = x0.numpy()
    info = np.finfo(np.float32)
    sub = (np.abs(x) < info.tiny) & (x != 0)
    assert x0.numel() == BC.CHUNK and sub.sum() >= 1000 and np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    assert (x == info.max).any() and (x == -info.max).any() and (x == info.tiny).any() and (x == -info.tiny).any()
    zero = x[x == 0]
    assert np.signbit(zero).any() and (~np.signbit(zero)).any()
    with np.errstate(all="ignore"):
        over = np.isfinite(x) & np.isinf(np.float32(BC.SPECIAL_COEFS[0]) * x)
    assert over.sum() >= 100


def test_the_operand_counts_stand_on_both_sides_of_every_kernarg_slot_size():
    assert BC.counts("step") == (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 80)
    assert BC.counts("masked") == (1, 4, 5, 8, 9, 12, 13, 16)
    assert BC.counts("backward") == (1, 4, 5, 8, 9, 16, 17, 80)
    assert BC.counts("masked_backward") == (1, 4, 5, 8, 9, 16)
    assert set(BC.TWO_OUT_PAIRS) <= set(BC.two_out_instantiated()) and any(nb == 1 for _, nb in BC.TWO_OUT_PAIRS) and any(nb == 0 for _, nb in BC.TWO_OUT_PAIRS)
    for k in BC.counts("step"):
        c = BC.random_coefs(k, "step")
        assert len(c) == k and (k < 3 or (c[1] == 0.0 and not np.signbit(c[1]))) and (k < 2 or any(v == 0.0 and np.signbit(v) for v in c))
        assert k < 2 or c[-1] != 0.0  # (the last fma is a live one: a fused convert behind it would show)


def test_same_bits_tells_signed_zeros_apart_and_nans_alike():
    a = torch.tensor([0.0, 1.0, float("nan")], dtype=torch.bfloat16)
    b = torch.tensor([-0.0, 1.0, float("nan")], dtype=torch.bfloat16)
    BM.same_bits(a, a.clone())
    BM.same_bits(torch.tensor([float("nan")]), torch.tensor([0x7FA00000], dtype=torch.int32).view(torch.float32))  # another NaN payload
    with pytest.raises(AssertionError, match="1 of 3 elements differ"):
        BM.same_bits(a, b, operands=(a,), what="zeros")
    with pytest.raises(AssertionError, match="1 of 1 elements differ"):
        BM.same_bits(torch.tensor([float("nan")]), torch.tensor([1.0]))


# ---- Runge-Kutta stage launches: div32, convert, rk_stage -----------------------------------------------------------------------------------
def exact_div_bits(a: np.float32, b: np.float32) -> int:
    "the fp32 bits of the exact quotient of two finite numbers, b != 0, rounded to nearest even; an exact zero has the quotient's sign"
    sign = int(np.signbit(a)) ^ int(np.signbit(b))
    return fl32_of_fraction(Fraction(float(a)) / Fraction(float(b)), sign)


def div_pairs():
    rng = np.random.default_rng(606)
    a, b = finite_patterns(rng, 2200), finite_patterns(rng, 2200)
    sets = [(a[b != 0], b[b != 0])]  # random bit patterns
    sets.append((scaled(rng, 2000, -100, -90), scaled(rng, 2000, 30, 50)))  # quotients in the subnormal range and just above and below it
    sets.append((scaled(rng, 1000, 60, 127), scaled(rng, 1000, -67, 0)))  # quotients around the overflow threshold
    sets.append((scaled(rng, 1000, -3, 3), scaled(rng, 1000, -3, 3)))
    top, tiny, one = np.float32(np.finfo(np.float32).max), np.float32(2.0**-149), np.float32(1)
    craft = [(top, np.float32(1 - 2.0**-24)), (top, np.float32(1 - 2.0**-23)), (top, one), (tiny, np.float32(2)), (np.float32(3 * 2.0**-149), np.float32(2)),
             (tiny, np.float32(-2)), (np.float32(2.0**-126), np.float32(1 + 2.0**-23)), (one, np.float32(3)), (np.float32(-0.0), one), (np.float32(0.0), np.float32(-3))]  # fmt: skip
    sets.append(tuple(np.array(col, dtype=np.float32) for col in zip(*craft)))
    return sets


def test_div32_is_the_correctly_rounded_quotient():
    checked = subnormal = 0
    for a, b in div_pairs():
        got = BM.div32(a, b).view(np.uint32)
        for i in range(a.size):
            want = exact_div_bits(a[i], b[i])
            assert int(got[i]) == want, (a[i], b[i], hex(int(got[i])), hex(want))
            subnormal += 0 < (want & 0x7FFFFFFF) < 0x00800000
        checked += a.size
    assert checked >= 6000 and subnormal >= 1500, (checked, subnormal)
    # zero, inf and NaN operands: IEEE's own rules, the sign of a zero or an inf included
    inf, nan, zero = np.float32(np.inf), np.float32(np.nan), np.float32(0)
    a = np.array([1, -1, 0, -0.0, 0, inf, -inf, inf, 1, -1, nan, 1, 0.0], dtype=np.float32)
    b = np.array([0, 0, 1, 2, 0, 2, -0.0, inf, inf, -inf, 1, nan, -0.0], dtype=np.float32)
    want = np.array([inf, -inf, zero, -zero, nan, inf, inf, nan, zero, zero, nan, nan, nan], dtype=np.float32)
    got = BM.div32(a, b)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])


STAGE_DTYPES = BC.STAGE_DTYPES
conversion_inputs = BC.conversion_inputs


@pytest.mark.parametrize("name", STAGE_DTYPES)
def test_convert_equals_cpu_torch_op_by_op(name):
    "all 15 kinds pairs: the model against table_cases.conversion_reference, which CPU torch evaluates one tensor op at a time in the dtype"
    dt = STAGE_DTYPES[name]
    elements = 0
    for what, s, o, ks in conversion_inputs(name):
        for k in ks:
            for kinds in BC.KINDS:
                ref = TC.conversion_reference(s, o, kinds, k)
                assert ref.dtype == dt
                BM.same_bits(BM.convert(dt, s, o, kinds, k), ref, operands=(s, o), what=f"{name} {what} kinds={kinds} k={k}")
                elements += s.numel()
    print(f"{name}: convert has CPU torch's bits on {elements} elements")


def test_the_stage_inputs_hold_what_the_issue_lists():
    assert BC.stage_slot_sizes() == [4, 8] and set(BC.STAGE_KS) == {4, 5, 2, 8}  # both sides of the slot size, and both ends
    assert len(BC.KINDS) == 15 and {op for kinds in BC.KINDS_FIVE for op in kinds} == {0, 1, 2, 3} and {f for _, f in BC.KINDS_FIVE} >= {0, 1, 2, 3}
    for name in BC.NARROW:
        (s, o), (o2, s2) = BC.conversion_patterns(name)
        assert s is s2 and o is o2 and np.array_equal(np.sort(BM.bits_of(o).astype(np.int64) & 0xFFFF), np.arange(65536)) and not torch.equal(s.view(torch.int16), o.view(torch.int16))
    s, o = (t.numpy() for t in BC.conversion_specials32())
    sp = BC._specials14()
    seen = {(int(a), int(b)) for a, b in zip(s.view(np.uint32)[:196], o.view(np.uint32)[:196])}
    assert len(sp) == 14 and seen == {(int(a), int(b)) for a in sp.view(np.uint32) for b in sp.view(np.uint32)} and s.size == BC.CHUNK
    k = [np.float32(v) for v in BC.SPECIALS_K]
    with np.errstate(all="ignore"):
        q = BM.div32(BM.sub32(s, BM.mul32(k[0], o)), k[1])
        assert ((np.abs(q) < np.finfo(np.float32).tiny) & (q != 0)).sum() >= 500  # quotients that underflow to subnormals
        assert (np.isinf(BM.mul32(k[0], o)) & np.isfinite(o)).sum() >= 300  # products that overflow
    for kk in BC.CONVERT_KS[1:]:
        assert min(kk) < 0 and any(np.frexp(abs(v))[0] == 0.5 for v in kk)
    for name in BC.NARROW:
        for K in BC.STAGE_KS:
            ops, coefs, chain, zeta1 = BC.stage_cancelling(name, K)
            assert len(ops) == len(coefs) == K and torch.equal(ops[0], ops[-1]) and (coefs[0], coefs[-1]) == (0.3, -0.3)
            assert all(abs(c) <= 3 * BC.STAGE_SCALE for c in (*coefs[1:-1], chain, zeta1))
        ops, coefs, chain, _, kinds, k = BC.stage_chain_cancels(name)
        assert coefs[1] == -chain and torch.equal(BM.convert(BC.DTYPES[name], ops[0], ops[1], kinds, k).view(torch.int16), ops[1].view(torch.int16))


# wrong variants of the conversion, on the host only: the operations of bit_model._convert with one of them replaced
class _Product:
    "k * o kept apart from its rounding, for the variants that fuse it with what follows"

    def __init__(self, a, b):
        self.a, self.b = a, b

    def real(self):
        return BM.mul32(self.a, self.b)


def convert_variant(dt: torch.dtype, s, o, kinds, k, variant: str) -> torch.Tensor:
    k = [np.float32(v) for v in k]
    plain = lambda v: v.real() if isinstance(v, _Product) else v  # noqa: E731
    rounded = lambda v: BM.widen(BM.round_to(dt, plain(v)))  # noqa: E731
    mul, sub, div, R = BM.mul32, BM.sub32, BM.div32, rounded
    if variant == "fused_product":  # the product and its rounding to the dtype as one instruction: the exact product, rounded once
        mul = _Product

        def R(v):
            if not isinstance(v, _Product):
                return rounded(v)
            if dt == torch.float16:
                with np.errstate(all="ignore"):
                    return BM.widen(round_once(dt, BM._wide(v.a) * BM._wide(v.b)))
            if dt == torch.bfloat16:  # bf16 is rounded by integer code on the bits of the fp32 product: there is nothing to fuse with
                bits = rne_bf16_bits(v.real().view(np.uint32)).astype(np.uint16)
                return BM.widen(torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16))
            return v.real()
    elif variant == "contracted":  # s - k * o as one fma: neither the product's fp32 rounding nor its rounding to the dtype
        mul = _Product
        R = lambda v: v if isinstance(v, _Product) else rounded(v)  # noqa: E731
        sub = lambda a, b: BM.fma32(-np.float32(b.a), b.b, a) if isinstance(b, _Product) and not isinstance(a, _Product) else BM.sub32(rounded(a), rounded(b))  # noqa: E731
        div = lambda a, b: BM.div32(rounded(a), b)  # noqa: E731
    elif variant == "reciprocal":
        div = lambda a, b: BM.mul32(a, BM.div32(np.float32(1), b))  # noqa: E731
    elif variant == "flushed":
        mul, sub, div = (lambda a, b, f=f: flush32(f(a, b), torch.float32) for f in (BM.mul32, BM.sub32, BM.div32))
    else:
        raise ValueError(variant)
    if variant == "contracted":  # (a product that nothing is subtracted from, or that is an operand of a further product, is a product)
        inner_mul = mul
        mul = lambda a, b: inner_mul(rounded(a) if isinstance(a, _Product) else a, rounded(b) if isinstance(b, _Product) else b)  # noqa: E731
    return BM.round_to(dt, rounded(BM._convert(BM.widen(s), BM.widen(o), kinds, k, mul, sub, div, R)))


HOLDS_PRODUCT_FIRST = [kd for kd in BC.KINDS if kd[0] != 0]  # to_x begins with a product
HOLDS_SUBTRACTION = [kd for kd in BC.KINDS if kd[0] == 1 or kd[1] == 1]  # s - k * o
DIVIDES = [kd for kd in BC.KINDS if kd[0] == 1 or kd[1] != 0]


def conversion_variant_counts(name: str, variant: str) -> dict:
    "{kinds: elements of the dtype's conversion inputs, over their k sets, where the variant's out0 has other bits than the model's}"
    dt = BC.DTYPES[name]
    n = {}
    for kinds in BC.KINDS:
        n[kinds] = 0
        for _, s, o, ks in conversion_inputs(name):
            for k in ks:
                n[kinds] += int(BM.differing(convert_variant(dt, s, o, kinds, k, variant), BM.convert(dt, s, o, kinds, k)).sum())
    return n


def show(n: dict) -> str:
    return " ".join(f"{t}{f}:{v}" for (t, f), v in n.items())


@pytest.mark.parametrize("name", ("bf16", "fp16", "fp32"))
def test_a_wrong_conversion_differs_from_the_model(name):
    n = {v: conversion_variant_counts(name, v) for v in ("fused_product", "contracted", "reciprocal", "flushed")}
    for v, counts in n.items():
        print(f"{name} {v}: {sum(counts.values())} elements differ, by kinds {show(counts)}")
    fused, contracted, reciprocal, flushed = (n[v] for v in ("fused_product", "contracted", "reciprocal", "flushed"))
    assert all(contracted[kd] == 0 for kd in BC.KINDS if kd not in HOLDS_SUBTRACTION) and all(reciprocal[kd] == 0 for kd in BC.KINDS if kd not in DIVIDES)
    assert sum(contracted[kd] for kd in HOLDS_SUBTRACTION) >= 500, contracted
    if name == "fp16":
        assert sum(fused[kd] for kd in HOLDS_PRODUCT_FIRST) >= 500, fused
    else:
        # bf16: pack_bf16 rounds with integer code on the bits of the fp32 product, no instruction multiplies and converts to bf16 -- the
        # "fused" form IS the model (here: an integer RNE written apart from torch's conversion).  fp32: there is no second rounding.
        assert sum(fused.values()) == 0, fused
    if name == "fp32":
        assert all(reciprocal[kd] >= 1000 for kd in DIVIDES), reciprocal
        # (a product, difference or quotient that is an fp32 subnormal: the specials hold 400 subnormal operands on either side, which
        # 0.9, -0.55 and 0.75 keep subnormal, and some 800 normals whose quotient by 3e38 is one)
        assert sum(flushed.values()) >= 1000, flushed
    else:
        # A 16-bit dividend has 2^10 (bf16: 2^7) significands, and the patterns hold every one of them against each divisor of CONVERT_KS.
        # The two quotients differ by a last place of fp32 at most; that survives the rounding to the dtype only if a / k lies within
        # 2^-23 of its size from a midpoint of the dtype, and none of these significands does for these divisors: the count is
        # exhaustive over them, not a sample.  Every 16-bit instantiation calls the div_ of the fp32 ones, which is where it is held.
        assert sum(reciprocal.values()) == 0, reciprocal
        if name == "fp16":  # (no fp32 subnormal arises from fp16 operands under these k: the smallest product is 2^-24 * 0.25)
            assert sum(flushed.values()) == 0, flushed
        else:  # (bf16 has fp32's exponents: its 254 subnormal patterns, and what they are multiplied into, are fp32 subnormals)
            assert sum(flushed.values()) >= 254, flushed


# wrong variants of out1, on the host only
def stage_variant(ops, coefs, chain, kinds, k, dt, zeta1=None, z1=None, variant=None) -> torch.Tensor:
    if variant is None:
        return BM.rk_stage(coefs, chain, ops, kinds, k, zeta1, z1)[1]
    d = BM.convert32(dt, ops[0], ops[1], kinds, k, keep_last=(variant == "unrounded_derivative"))
    terms = [(np.float32(c), BM.widen(x)) for c, x in zip(coefs, ops)]
    chained = [(np.float32(chain), d)]
    noise = [(np.float32(zeta1), BM.widen(z1))] if zeta1 is not None and np.float32(zeta1) != 0 else []
    order = {"chain_first": chained + terms + noise, "reversed": terms[::-1] + chained + noise, "noise_first": terms + noise + chained}.get(variant, terms + chained + noise)
    fma = mul_add if variant == "mul_add" else BM.fma32
    s1 = np.zeros(terms[0][1].shape, dtype=np.float32)
    for c, x in order:
        s1 = fma(c, x, s1)
    return BM.round_to(dt, s1)


STAGE_VARIANTS = ("unrounded_derivative", "chain_first", "reversed", "mul_add", "noise_first")


def stage_variant_counts(name: str, variant: str) -> dict:
    "elements of out1 where the variant has other bits than the model, over the stage inputs: stage_cancelling at every K, stage_chain_cancels"
    dt = BC.DTYPES[name]
    z = host_normal(BC.SAMPLES * BC.SAMPLE)
    n = {}
    for K in BC.STAGE_KS:
        ops, coefs, chain, zeta1 = BC.stage_cancelling(name, K)
        for noisy in (False, True):
            args = (ops, coefs, chain, (1, 2), BC.CONVERT_KS[0], dt) + ((zeta1, z) if noisy else (None, None))
            n[f"cancelling K={K}{' noisy' if noisy else ''}"] = int(BM.differing(stage_variant(*args, variant=variant), stage_variant(*args)).sum())
    ops, coefs, chain, zeta1, kinds, k = BC.stage_chain_cancels(name)
    args = (ops, coefs, chain, kinds, k, dt, zeta1, z)
    n["chain_cancels noisy"] = int(BM.differing(stage_variant(*args, variant=variant), stage_variant(*args)).sum())
    return n


@pytest.mark.parametrize("variant", STAGE_VARIANTS)
@pytest.mark.parametrize("name", BC.NARROW)
def test_a_wrong_stage_differs_from_the_model_16_bit(name, variant):
    n = stage_variant_counts(name, variant)
    print(f"{name} {variant}: {sum(n.values())} of {(2 * len(BC.STAGE_KS) + 1) * BC.SAMPLES * BC.SAMPLE} elements differ {n}")
    assert sum(n.values()) >= 200, (name, variant, n)
    if variant == "noise_first":  # (behind the self-cancelling s the chain and the noise are both small terms: only the chain as the canceller tells their order)
        assert n["chain_cancels noisy"] >= 200, n
