"""The exact model of the step kernels' fp32 arithmetic (tests/bit_model.py) and its inputs (tests/bit_cases.py), checked on the host:

  * the model is right: fma32 against exact rational arithmetic, round_to against an integer round-to-nearest-even on the bit patterns;
  * the inputs are sharp: TIES and PATTERNS hold the classes of elements at which a wrong kernel gives other bits, counted from the model;
  * the tests can fail: six wrong variants of the contract, built on the host only, each differ from the model on many elements.

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
