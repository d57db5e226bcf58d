"""Inputs of tests/test_bit_model_host.py and tests/test_bit_contract_gpu.py: the operand sets at which a step kernel that breaks the
fp32 accumulate-and-round contract (tests/bit_model.py) cannot keep the contract's bits, and the operand counts read off the sources.

  PATTERNS  all 65 536 bit patterns of a 16-bit dtype as operand 0: every NaN, both infs, every subnormal, both zeros.
  TIES      for every finite non-zero pattern a whose distance u to the next pattern away from zero is itself a value of the dtype
            (and whose next pattern is finite): operands (a, u, u), coefficients (1, 0.5, k3).  k3 = 0 is an exact 16-bit tie in
            fp32; +-2^-12 lies just off it, exactly; +-2^-18 makes the last fma inexact, so that the fp32 VALUE lands on the tie
            while the exact sum does not -- where a fused multiply-add-and-convert, which rounds the exact sum once, gives other bits.
            The two top patterns of each sign follow: their tie is the overflow threshold and rounds to inf.
  RANDOM    4 samples of 3 chunks of seeded normals at the operand scales of table_cases.pool, coefficients as table_cases._coef
            with one exact zero and one -0.0, at the operand counts on both sides of every kernarg slot size.
  SPECIALS  fp32 only: +-0, +-inf, NaN, +-max, +-smallest normal, 1 000 subnormals, numbers whose product with a coefficient overflows.
  cancelling sums (mixed_operands, masked_cancelling): RANDOM with one fp32 operand chosen so that the result is rounding residue.  Among
            unrelated normals a last-place difference of the fp32 value survives the rounding to a 16-bit output once in 2^15; here a
            split fma or another order shows in most elements.

  stage launches (conversion_inputs, stage_cancelling, stage_chain_cancels): for the rounded conversion, every pattern of a 16-bit dtype
            as s against a permutation as o and the reverse, under two sets of k; fp32 normals and a chunk of specials whose products
            overflow and whose quotients underflow.  For out1, an s that cancels itself (coefficients 0.3 and -0.3 at both ends, all
            else scaled by 2^-16) and a chain that cancels coef1[1]: the order of the operands, of the chain and of the noise, and a
            split fma, show through a 16-bit output in thousands of elements.

Every set is padded with 1.0 to whole 2048-element chunks.  `ragged` adds three elements for the launches that must miss the
whole-chunk kernels; they repeat elements of the set instead of 1.0, so that the scalar tail of a grid-stride kernel rounds ties too.
Nothing in this module needs a GPU."""

from __future__ import annotations

import functools
import os
import random
import re

import bit_model as BM
import numpy as np
import torch

from skrample_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 2048
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NARROW = ("bf16", "fp16")
SAMPLES, SAMPLE = 4, 3 * CHUNK  # RANDOM: 4 samples of 3 chunks
TIE_K3 = (0.0, 2.0**-12, -(2.0**-12), 2.0**-18, -(2.0**-18))
TIE_COEFS = (1.0, 0.5)
SCALES = (1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 3.0, 1.0, 0.125, 2.5, 1.0, 0.5, 4.0, 1.25, 0.3, 1.75)  # table_cases.pool


# ---- operand counts, read from the sources ---------------------------------------------------------------------------------------------
def _source(name: str) -> str:
    return open(os.path.join(ROOT, "skrample_amd", "csrc", name)).read()


def ladder(file: str, func: str) -> list[int]:
    "the kernarg slot sizes of `constexpr int func(int k) { return k <= A ? A : (k <= B ? B : ... TOP); }`"
    body = re.search(rf"constexpr int {func}\(int \w+\) \{{ return (.*?); \}}", _source(file)).group(1)
    sizes = [int(x) for x in re.findall(r"<= (\d+) \?", body)]
    return sizes + [int(re.search(r"(\d+)\)*$", body).group(1))]


def around(sizes: list[int], top: int) -> tuple[int, ...]:
    "1, both sides of every slot size, and the family's maximum"
    return tuple(sorted({1, top} | {k for s in sizes for k in (s, s + 1) if k <= top}))


@functools.lru_cache(maxsize=None)
def counts(family: str) -> tuple[int, ...]:
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    max_terms = int(re.search(r"#define SKR_MAX_TERMS (\d+)", header).group(1))
    row_terms = int(re.search(r"#define SKR_ROW_TERMS (\d+)", header).group(1))
    assert (max_terms, row_terms) == (_hip.MAX_TERMS, _hip.ROW_TERMS)
    if family == "step":  # one-trip kernels up to ONE_TRIP_MAX_K operands, the general kernel beyond
        one_trip = ladder("skr_step_fast.hip", "one_trip_kmax")
        assert one_trip[-1] == int(re.search(r"constexpr int ONE_TRIP_MAX_K = (\d+);", _source("skr_step_fast.hip")).group(1))
        return around(one_trip, max_terms)
    if family == "masked":
        sizes = ladder("skr_step_masked.hip", "masked_kmax")
        assert sizes[-1] == row_terms
        return around(sizes[:-1], row_terms)
    body = re.search(r"static void with_bwd_k1\(.*?\n\}", _source("skr_step_backward.hip"), re.S).group(0)
    sizes = [int(x) for x in re.findall(r"p\.n_grads <= (\d+)", body)]
    top = max(int(x) for x in re.findall(r"integral_constant<int, (\d+)>", body))
    assert sizes and top == int(re.search(r"p\.n_grads <= (\d+) && numel % CHUNK", _source("skr_step_backward.hip")).group(1))
    if family == "backward":  # one-trip up to `top` gradients, the general kernel beyond
        return around(sizes + [top], max_terms)
    assert family == "masked_backward" and top == row_terms
    return around(sizes, row_terms)


TWO_OUT_PAIRS = ((4, 0), (4, 1), (8, 1))  # (NA, NB) of step_kernel_k2: 4, 5 and 9 kernarg slots' worth, one without an fp32 operand


def two_out_instantiated() -> list[tuple[int, int]]:
    listed = re.search(r"using TwoOutCounts = TwoOutList<(.*?)>;", _source("skr_step_fast.hip"), re.S).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"TwoOut<(\d+), (\d+), \w+>", listed)]


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def pad(t: torch.Tensor) -> torch.Tensor:
    "padded with 1.0 to whole chunks"
    n = -t.numel() % CHUNK
    return torch.cat([t.reshape(-1), torch.ones(n, dtype=t.dtype)]) if n else t.reshape(-1).clone()


def ragged(t: torch.Tensor) -> torch.Tensor:
    """three elements more than whole chunks: a quarter into the set (in PATTERNS and TIES three neighbouring positive normal patterns, so
    ties towards an even and towards an odd pattern), the same three positions for every operand"""
    at = t.numel() // 4
    return torch.cat([t, t[at : at + 3]])


# ---- PATTERNS -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def patterns(name: str) -> torch.Tensor:
    "all 65 536 bit patterns of a 16-bit dtype, pattern p at index p"
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(DTYPES[name])


# ---- TIES -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ties(name: str):
    "(a, u) in the dtype, padded to whole chunks, and the number of elements in front of the padding"
    dt = DTYPES[name]
    pats = patterns(name)
    a32 = pats.float()
    nxt = (pats.view(torch.int16) + 1).view(dt).float()  # the next pattern away from zero (finite non-zero patterns keep their sign)
    u32 = nxt - a32  # exact: neighbours
    keep = torch.isfinite(a32) & (a32 != 0) & torch.isfinite(nxt) & (u32.to(dt).float() == u32)
    a, u = pats[keep], u32[keep].to(dt)
    # the two top patterns of each sign: a + u/2 is the tie between them (top but one) and the overflow threshold (top)
    info = torch.finfo(dt)
    top = torch.tensor([info.max], dtype=dt)
    below = (top.view(torch.int16) - 1).view(dt)
    step = (top.float() - below.float()).to(dt)
    extra_a = torch.cat([below, top, -below, -top])
    extra_u = torch.cat([step, step, -step, -step])
    a, u = torch.cat([a, extra_a]), torch.cat([u, extra_u])
    return pad(a), pad(u), a.numel()


def tie_operands(name: str, wide_u: bool = False):
    "(a, u, u); wide_u: u carried as fp32 (the mixed-group launches)"
    a, u, _ = ties(name)
    u = u.float() if wide_u else u
    return [a, u, u.clone()]


def tie_coefs(k3: float) -> list[float]:
    return [*TIE_COEFS, k3]


# ---- RANDOM ---------------------------------------------------------------------------------------------------------------------------
def _coef(rng: random.Random) -> float:  # table_cases._coef
    c = (1.0, -1.0, rng.uniform(-3, 3), rng.uniform(-1e-2, 1e-2))[rng.randrange(4)]
    return c if c != 0.0 else 0.5


def random_coefs(k: int, salt: str) -> list[float]:
    """k coefficients: +-1, uniform(-3, 3), uniform(-1e-2, 1e-2); from two operands on one is -0.0 (the first; from four on the middle
    one), from three on the second is 0.0.  The last is never zero: the fma in front of the rounding is a live one."""
    rng = random.Random(f"bits/{salt}/{k}")
    c = [_coef(rng) for _ in range(k)]
    if k >= 2:
        c[k // 2 if k >= 4 else 0] = -0.0
    if k >= 3:
        c[1] = 0.0
    return c


def masked_coef1(k: int) -> list[float]:
    "the known form of a masked step: zeros of both signs (operands that are not part of it) and two or three live coefficients at the end and in the middle"
    rng = random.Random(f"bits/known/{k}")
    c = [0.0 if j % 2 else -0.0 for j in range(k)]
    for j in {k - 1, max(k - 2, 0), k // 2}:
        c[j] = _coef(rng)
    return c


@functools.lru_cache(maxsize=8)
def random_operands(name: str, k: int, salt: str = "x") -> tuple:
    "k operands of SAMPLES * SAMPLE elements; the first 64 elements of every sample of operand 0 are exact zeros (signed-zero sums)"
    g = torch.Generator().manual_seed(random.Random(f"bits/{name}/{k}/{salt}").randrange(2**31))
    ops = [(torch.randn(SAMPLES * SAMPLE, generator=g) * SCALES[j % len(SCALES)]).to(DTYPES[name]) for j in range(k)]
    ops[0].view(SAMPLES, SAMPLE)[:, :64] = 0
    return tuple(ops)


MIXED_KS = (2, 5, 9)  # operands of a mixed-group launch, the fp32 one last


def mixed_operands(name: str, k: int, zeta=None, z=None) -> tuple:
    """k - 1 operands of the 16-bit dtype and one fp32 operand behind them, with coefficients.  In the first two samples the fp32 operand is
    normal; in the last two it is fl32(-(s + zeta z) / c), s the contract's sum of the others, c its own coefficient and zeta z the noise
    the launch adds behind it (none: 0), so that the result is nothing but rounding residue: any other order or rounding of the fp32
    operations shows in most elements of a 16-bit output, where among unrelated normals a last-place difference of the fp32 value
    survives the rounding once in 2^15."""
    narrow = random_operands(name, k - 1, "mixed")
    coefs = random_coefs(k, "mixed")
    g = torch.Generator().manual_seed(4242 + k)
    wide = torch.randn(SAMPLES * SAMPLE, generator=g) * 1.5
    s = BM.step32(coefs[:-1], narrow).astype(np.float64)
    if zeta is not None and z is not None:
        s = s + float(np.float32(zeta)) * BM.widen(z).astype(np.float64)
    with np.errstate(all="ignore"):
        cancel = torch.from_numpy((-s / float(np.float32(coefs[-1]))).astype(np.float32))
    wide[2 * SAMPLE :] = cancel[2 * SAMPLE :]
    return (*narrow, wide), coefs


def masked_cancelling(name: str, k: int, mask_flat: torch.Tensor) -> tuple:
    """A masked step whose two blended terms cancel: k - 1 operands of the 16-bit dtype and one fp32 operand that takes part in the known
    form alone (coef0 0, coef1 1) and is chosen, element by element, so that (1 - m) k = -m s up to rounding.  The output is rounding
    residue, as in mixed_operands, and a blend computed as two products and an add shows in most elements.  `mask_flat`: the mask element
    of every element.  Where m is 0 or 1 the fp32 operand is normal.  Returns (operands, coef0, coef1)."""
    narrow = random_operands(name, k - 1, "known")
    c0, c1 = random_coefs(k - 1, "masked0") + [0.0], masked_coef1(k - 1) + [1.0]
    m = BM.widen(mask_flat).astype(np.float64)
    s = BM.step32(c0[:-1], narrow).astype(np.float64)
    kn = BM._accumulate(c1[:-1], narrow, skip_zero=True).astype(np.float64)
    g = torch.Generator().manual_seed(977 + k)
    wide = torch.randn(SAMPLES * SAMPLE, generator=g)
    with np.errstate(all="ignore"):
        x = (-m * s / (1 - m) - kn).astype(np.float32)
    soft = torch.from_numpy((m > 0) & (m < 1) & np.isfinite(x))
    wide[soft] = torch.from_numpy(x)[soft]
    return (*narrow, wide), c0, c1


# ---- SPECIALS (fp32) ------------------------------------------------------------------------------------------------------------------
SPECIAL_COEFS = (3.0, -0.75)  # 3 * max and 3 * 1.2e38 overflow in the product; -0.75 * a subnormal is inexact


@functools.lru_cache(maxsize=None)
def specials32() -> tuple:
    "two fp32 operands of one chunk: the special values against each other (operand 1 is operand 0 rolled by 7)"
    info = np.finfo(np.float32)
    rng = np.random.default_rng(77)
    sub = rng.integers(1, 2**23, 1000, dtype=np.uint32) | (rng.integers(0, 2, 1000, dtype=np.uint32) << np.uint32(31))
    head = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, info.max, -info.max, info.tiny, -info.tiny], dtype=np.float32)
    big = (rng.uniform(1.14e38, 3.4e38, 300) * rng.choice([-1.0, 1.0], 300)).astype(np.float32)  # times 3: beyond max
    plain = rng.standard_normal(CHUNK).astype(np.float32)
    x0 = np.concatenate([head, sub.view(np.float32), big, np.tile(head, 8), plain])[:CHUNK].copy()
    x1 = np.roll(x0, 7)
    return torch.from_numpy(x0), torch.from_numpy(x1.copy())


# ---- Runge-Kutta stage launches -------------------------------------------------------------------------------------------------------
KINDS = tuple((t, f) for t in range(4) for f in range(4) if (t, f) != (0, 0))  # the 15 rounded conversions
KINDS_FIVE = ((1, 0), (2, 0), (3, 3), (0, 1), (0, 2))  # between them every operation of convert_rounded
# (k0 .. k3): the constants of tests/test_step_gpu.py::test_rounded_conversion_equals_torch_op_by_op; a negative k0 (as
# table_cases.CONVERT_K row 3) with a power of two as k1, which divides in to_x kind 1 and multiplies in kind 2
CONVERT_KS = ((0.9, 0.09999999999999998, 0.7310585786300049, 0.35), (-0.55, 0.25, 0.8810585786300049, 0.53))
# fp32 specials: 3 * FLT_MAX overflows in the product, anything / 3e38 below 3.5 is a subnormal quotient, FLT_MIN * 0.75 a subnormal product
SPECIALS_K = (3.0, 3e38, 0.75, 3e38)
STAGE_KS = (2, 4, 5, 8)  # operands on both sides of the kernarg slot size of RkOneTripArgs
STAGE_SCALE = 2.0**-16
STAGE_ZETA = 0.625


def stage_slot_sizes() -> list[int]:
    "the kernarg slot sizes of step_kernel_rk1, `RkOneTripArgs<(K <= A ? A : B)>`, and the operand counts its launcher instantiates"
    src = _source("skr_step_fast.hip")
    a, a2, b = re.search(r"void step_kernel_rk1\(const RkOneTripArgs<\(K <= (\d+) \? (\d+) : (\d+)\)> a\)", src).groups()
    assert a == a2
    lo, hi = re.search(r"static int launch_rk1\(.*?with_count<(\d+), (\d+)>\(args\.n_terms", src, re.S).groups()
    assert (int(lo), int(hi)) == (2, int(b)), (lo, hi, b)
    return [int(a), int(b)]


@functools.lru_cache(maxsize=None)
def conversion_patterns(name: str) -> tuple:
    "((s, o), (o, s)): s all 65 536 patterns of the dtype, o a fixed permutation of them"
    s = patterns(name)
    o = s[torch.randperm(65536, generator=torch.Generator().manual_seed(1492))].clone()
    return (s, o), (o, s)


def _specials14() -> np.ndarray:
    info = np.finfo(np.float32)
    sub = np.array([1, 0x7FFFFF], dtype=np.uint32).view(np.float32)  # the smallest and the largest subnormal
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub[0], -sub[0], sub[1], -sub[1], info.tiny, -info.tiny, info.max, -info.max, 1.0], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def conversion_specials32() -> tuple:
    """(s, o), one chunk of fp32: the 14 x 14 block of (+-0, +-inf, NaN, the smallest and the largest subnormal of both signs, +-FLT_MIN,
    +-FLT_MAX, 1) against each other, both ways round; 400 subnormals beside normals and 400 normals beside subnormals; 300 numbers beyond
    FLT_MAX / 3 beside normals, and the reverse; numbers within a factor 4 of FLT_MIN beside each other; normals"""
    sp = _specials14()
    rng = np.random.default_rng(1777)
    sub = (rng.integers(1, 2**23, 400, dtype=np.uint32) | (rng.integers(0, 2, 400, dtype=np.uint32) << np.uint32(31))).view(np.float32)
    big = (rng.uniform(1.14e38, 3.4e38, 300) * rng.choice([-1.0, 1.0], 300)).astype(np.float32)
    small = (rng.uniform(1.0, 4.0, 200) * np.finfo(np.float32).tiny * rng.choice([-1.0, 1.0], 200)).astype(np.float32)
    nrm = lambda n: rng.standard_normal(n).astype(np.float32)  # noqa: E731
    s = np.concatenate([np.repeat(sp, 14), sub, nrm(400), big, nrm(300), small, nrm(CHUNK)])[:CHUNK].copy()
    o = np.concatenate([np.tile(sp, 14), nrm(400), sub, nrm(300), big, small[::-1], nrm(CHUNK)])[:CHUNK].copy()
    return torch.from_numpy(s), torch.from_numpy(o)


@functools.lru_cache(maxsize=None)
def stage_extras(name: str, n: int, count: int = 7) -> tuple:
    "`count` operands of n seeded normals at the scales of table_cases.pool: what stands behind a conversion's pair in a stage launch"
    g = torch.Generator().manual_seed(random.Random(f"bits/stage/{name}/{n}").randrange(2**31))
    return tuple((torch.randn(n, generator=g) * SCALES[(j + 2) % len(SCALES)]).to(DTYPES[name]) for j in range(count))


STAGE_DTYPES = {**DTYPES, "fp64": torch.float64}


def conversion_inputs(name: str) -> list:
    """[(what, s, o, k sets)], the conversion inputs of one dtype.  16-bit: the patterns both ways round under CONVERT_KS.  fp32 (and fp64:
    the same numbers widened): SAMPLES * SAMPLE seeded normals under CONVERT_KS, the specials under CONVERT_KS and SPECIALS_K."""
    if name in NARROW:
        return [(f"patterns {i}", s, o, CONVERT_KS) for i, (s, o) in enumerate(conversion_patterns(name))]
    s, o = random_operands("fp32", 2, "cancel")
    sp = conversion_specials32()
    dt = STAGE_DTYPES[name]
    return [("normals", s.to(dt), o.to(dt), CONVERT_KS), ("specials", sp[0].to(dt), sp[1].to(dt), (*CONVERT_KS, SPECIALS_K))]


def stage_coefs(k: int, salt: str = "stage") -> list[float]:
    "coef1 of a stage over unrelated operands: random_coefs (a -0.0 and, from three operands on, a 0.0 among them)"
    return random_coefs(k, salt)


def stage_operands(name: str, pair: tuple, k: int) -> tuple:
    "a conversion's pair with k - 2 operands of seeded normals behind it"
    return (*pair, *stage_extras(name, pair[0].numel())[: k - 2])


def stage_cancelling(name: str, k: int, scale: float = STAGE_SCALE) -> tuple:
    """(operands, coef1, chain, zeta1): operand 0 (s) has coefficient 0.3 and the last operand is the same tensor with coefficient -0.3
    (k = 2: o is s), so that fma(-0.3, s, ... fl32(0.3 s)) leaves the rounding residue of the first product.  Every other coefficient, the
    chain and zeta1 carry `scale`: all that stands between the two is of the residue's size, and another order of the operands, a chain
    in front of them or a product rounded apart from its sum shows through a 16-bit output in thousands of elements (among unrelated
    normals: once in 2^15).  SAMPLES * SAMPLE elements, s and o seeded normals."""
    s, o = random_operands(name, 2, "cancel")
    mid = stage_extras(name, s.numel())[: max(k - 3, 0)]
    ops = (s, s.clone()) if k == 2 else (s, o, *mid, s.clone())
    rng = random.Random(f"bits/cancel/{k}")
    coefs = [0.3] + [rng.uniform(0.5, 3) * rng.choice([-1, 1]) * scale for _ in range(k - 2)] + [-0.3]
    return ops, coefs, -0.4375 * scale, STAGE_ZETA * scale


def stage_chain_cancels(name: str, scale: float = STAGE_SCALE) -> tuple:
    """(operands, coef1, chain, zeta1, kinds, k) for the order of the last two fmas: kinds (3, 0) with k0 = 1 make the derivative o bit for
    bit, and coef1[1] = -chain, so the chain fma cancels the sum down to what the scaled terms (s, a third operand, the noise) left.
    A noise fma in front of the chain's is rounded at the size of chain * o instead."""
    s, o = random_operands(name, 2, "cancel")
    (w,) = stage_extras(name, s.numel())[:1]
    chain = 0.8125
    return (s, o, w), [1.25 * scale, -chain, -0.75 * scale], chain, STAGE_ZETA * scale, (3, 0), (1.0, 1.0, 1.0, 1.0)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def mask_values(dt: torch.dtype) -> torch.Tensor:
    "0, 1, 0.5, the two neighbours of 1 and of 0.5, the smallest subnormal"
    one, half = torch.tensor([1.0], dtype=dt), torch.tensor([0.5], dtype=dt)
    bits = torch.int16 if dt != torch.float32 else torch.int32
    near = [(v.view(bits) + d).view(dt) for v in (one, half) for d in (-1, 1)]
    tiny = torch.tensor([1], dtype=bits).view(dt)
    return torch.cat([torch.zeros(1, dtype=dt), one, half, *near, tiny])


def soft_mask(dt: torch.dtype, samples: int, mask_numel: int, seed: int) -> torch.Tensor:
    "[samples, mask_numel] of dtype values in [0, 1] (and the neighbour above 1): uniform, with mask_values at the front and every 97th element"
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(samples, mask_numel, generator=g).to(dt)
    vals = mask_values(dt)
    m[:, : vals.numel()] = vals
    at = torch.arange(vals.numel() + 5, mask_numel, 97)
    m[:, at] = vals[torch.arange(at.numel()) % vals.numel()]
    return m


def expand_mask(mask: torch.Tensor, batch_stride: int, samples: int, sample: int) -> torch.Tensor:
    "the mask element every element of the launch reads: mask[smp * batch_stride + r % mask_numel], flat"
    mask_numel = mask.shape[-1]
    rows = mask.reshape(-1, mask_numel)
    rows = rows if batch_stride else rows[:1].expand(samples, mask_numel)
    assert rows.shape[0] == samples and sample % mask_numel == 0
    return rows.repeat(1, sample // mask_numel).reshape(-1)
