"""Which axis lengths the own any-length transforms (csrc/skr_fft_own.hip) take, how they take them, and a float64 reference of
skr_colorize: helper of tests/test_fft_lengths_host.py, tests/test_fft_lengths_gpu.py and tests/test_noise_gpu.py.  Nothing here needs a GPU.

The predicates restate the PROSE of the file's header and of include/skrample_hip.h, not the code: every axis length up to 2048
(Bluestein), up to 4096 the direct ones -- a power of two, or 2^a (a >= 1) times at most three factors out of 3, 5, 7, 11, 13 -- and, as
the LAST axis, any even length 2 A B with A, B such lengths.  `classify` adds HOW a length is served (which direct form, which
Bluestein size, which split), `tile_lines` how many lines share a tile.  The three constants the prose assumes are read from the
sources and asserted, so that a change of one of them fails here first.

`colorize64` is oracle/skr_oracle/noise.py::colorize on numpy float64, per sample: torch's CPU FFT is not used for sweeps of thousands
of lengths (tests/test_fft_lengths_host.py pins the restatement to the oracle at a dozen shapes)."""

from __future__ import annotations

import functools
import os
import re

import numpy as np
import torch
from skr_oracle import noise as ON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (13, 11, 7, 5, 3)
EXPONENTS = (0.25, -1.4, 1.7)
ENERGY, ENERGY_EVERY = 2.5, 16
SHIFT = 0.25  # added to the second sample of every call: a live DC bin
ROLES = ("only", "last", "outer", "middle")
BAR = 1e-5  # tests/test_noise_gpu.py::COLORED_TOL, the generator bar (profiles/r04_parity_margins.txt)


def _source(name: str) -> str:
    return open(os.path.join(ROOT, "skrample_amd", "csrc", name)).read()


@functools.lru_cache(maxsize=None)
def constants() -> dict:
    "OWN_MAX_M, FFT_MAX_TILE and FFT_THREADS as the sources define them; the values the prose (and everything below) assumes"
    got = {
        "OWN_MAX_M": int(re.search(r"constexpr int OWN_MAX_M = (\d+);", _source("skr_fft_own.hip")).group(1)),
        "FFT_MAX_TILE": int(re.search(r"constexpr int FFT_MAX_TILE = (\d+);", _source("skr_fft_tile.h")).group(1)),
        "FFT_THREADS": int(re.search(r"constexpr int FFT_THREADS = (\d+);", _source("skr_fft_tile.h")).group(1)),
    }
    assert got == {"OWN_MAX_M": 4096, "FFT_MAX_TILE": 4096, "FFT_THREADS": 256}, got
    return got


# ---- the predicates (moved here from tests/test_noise_gpu.py) ----------------------------------------------------------------------------
def _short_length(d: int) -> bool:
    "an axis length the tile transforms of skr_fft_own.hip take: anything up to 2048 (Bluestein), and up to 4096 the direct ones -- 2^a (a >= 1) times at most three factors out of 3, 5, 7, 11, 13"
    if d <= 2048:
        return True
    if d > 4096:  # (the version in tests/test_noise_gpu.py compared what was left of d after the odd factors: 4160 = 2^6 5 13 passed)
        return False
    odd = 0
    for f in (13, 11, 7, 5, 3):
        while d % f == 0 and odd < 3:
            d, odd = d // f, odd + 1
    return d & (d - 1) == 0 and (odd == 0 or d >= 2)


def _own_length(d: int, last: bool = False) -> bool:
    "... or, as the LAST axis, an even length 2 A B with A, B such lengths (the half-length transform in four steps)"
    if _short_length(d):
        return True
    h = d // 2
    return last and d % 2 == 0 and any(h % a == 0 and _short_length(a) and _short_length(h // a) for a in range(2, int(h**0.5) + 1))


# ---- how a length is served --------------------------------------------------------------------------------------------------------------
def direct_form(n: int):
    "(p, radix multiset) when n = p r is a direct form -- p = 2^a, a >= 1, r a product of at most three of 3, 5, 7, 11, 13 (none: a power of two) -- else None"
    rads, rest = [], n
    for f in FACTORS:
        while rest % f == 0 and len(rads) < 3:
            rads.append(f)
            rest //= f
    if rest >= 2 and rest & (rest - 1) == 0 and n <= constants()["OWN_MAX_M"]:
        return rest, tuple(sorted(rads))
    return None


def bluestein_size(n: int) -> tuple[int, int]:
    """(m, r): m = r p >= 2 n - 1 with p a power of two and r = 1, 3 or 5, whichever is cheapest -- p log2 p butterflies per segment
    plus 2.5 passes' worth for the radix-r pass; the first of equals in the order r = 1, 3, 5 (the header's "130 points: 320 instead of 512")"""
    best, pick = None, None
    for r in (1, 3, 5):
        p = 2
        while p * r < 2 * n - 1:
            p *= 2
        if p * r > constants()["OWN_MAX_M"]:
            continue
        cost = p * r * (p.bit_length() - 1 + (2.5 if r > 1 else 0.0))
        if best is None or cost < best:
            best, pick = cost, (p * r, r)
    assert pick is not None, n
    return pick


def _loosely_direct(m: int) -> bool:
    """what own_long_split's scoring calls direct: up to three of EACH odd factor stripped, and nothing but 1 left counts as well -- so 9, 25,
    1125 = 3^2 5^3 or 3003 pass, which own_axis (and the header's prose) send through Bluestein.  Only the preference is affected, not
    which lengths are accepted; kept here so that the tests can tell where the two readings pick different factors."""
    for f in FACTORS:
        for _ in range(3):
            if m % f == 0:
                m //= f
    return m & (m - 1) == 0


def long_split(n: int, loose: bool = False):
    """(A, B), n = 2 A B: both short lengths, direct forms preferred over Bluestein, then as close to each other as they come (A <= B).
    `loose`: with the scoring's own reading of "direct" (_loosely_direct) instead of the documented one"""
    if n < 4 or n % 2:
        return None
    is_direct = _loosely_direct if loose else (lambda m: direct_form(m) is not None)
    h, best, pick = n // 2, -1, None
    for a in range(2, int(h**0.5) + 1):
        if h % a == 0 and a * a <= h and _short_length(a) and _short_length(h // a):
            score = (2 * 4096) * (is_direct(a) + is_direct(h // a)) + a
            if score > best:
                best, pick = score, (a, h // a)
    return pick


def classify(n: int, last: bool = False) -> tuple:
    """("direct", p, rads) | ("bluestein", m, r) | ("long", A, B) | ("refused",) for an axis of n points (`last`: the innermost, real axis)"""
    if n >= 2 and _short_length(n):
        form = direct_form(n)
        return ("direct", *form) if form else ("bluestein", *bluestein_size(n))
    split = long_split(n) if last and n >= 2 else None
    return ("long", *split) if split else ("refused",)


def class_name(c: tuple) -> str:
    if c[0] == "direct":
        return "direct " + ("x".join(map(str, c[2])) if c[2] else "2^a")
    if c[0] == "bluestein":
        return f"bluestein m={c[1]} r={c[2]}"
    return c[0]


def transform_size(c: tuple) -> int:
    "m of a short length's class: the points of one line in the tile"
    assert c[0] in ("direct", "bluestein")
    return c[1] * int(np.prod(c[2], dtype=np.int64)) if c[0] == "direct" else c[1]


def full_tile(m: int) -> int:
    "the most lines of m points one tile takes: a power of two, at most FFT_MAX_TILE points and FFT_THREADS lines"
    k, L = constants(), 1
    while 2 * L * m <= k["FFT_MAX_TILE"] and 2 * L <= k["FFT_THREADS"]:
        L *= 2
    return L


def tile_lines(m: int, lines: int) -> int:
    """logical lines per block, from the source's rule: the full tile, halved while the launch has fewer than two blocks for each of the
    256 CUs and half the tile still gives every thread two points"""
    L = full_tile(m)
    while L > 1 and -(-lines // L) < 2 * 256 and (L // 2) * m >= 2 * constants()["FFT_THREADS"]:
        L //= 2
    return L


# ---- the sweep's units and inputs --------------------------------------------------------------------------------------------------------
def role_dims(role: str, n: int) -> tuple:
    return {"only": (n,), "last": (3, n), "outer": (n, 4), "middle": (3, n, 4)}[role]


def role_accepts(role: str, n: int) -> bool:
    return _own_length(n, last=role in ("only", "last"))


def exponent_of(n: int) -> float:
    return EXPONENTS[n % 3]


def energy_of(n: int):
    return ENERGY if n % ENERGY_EVERY == 0 else None


def white_input(role: str, dims, batch: int = 2) -> torch.Tensor:
    "the fp32 white noise of one call, [batch, *dims]: seeded per (role, dims); every sample but the first shifted by SHIFT"
    seed = (ROLES.index(role) if role in ROLES else len(ROLES) + sum(map(ord, role))) * 1_000_003 + int(np.prod(dims, dtype=np.int64)) * 31 + len(dims)
    w = torch.randn((batch, *dims), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    w[1:] += SHIFT
    return w


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def _weights(unit: tuple, exponent: float) -> np.ndarray:
    "ON.colorize's spectral weights, computed as it computes them (tests/test_colored_whole_batch_gpu.py::weights64)"
    grid = ON.radial_freq_grid(unit)
    clip = 0.5 / max(sum(unit) / len(unit), 4.0)
    return (torch.clamp(grid, min=clip) ** (-exponent / 2.0)).numpy()


def colorize_np(white: np.ndarray, exponent: float, energy, dtype=np.float64) -> np.ndarray:
    """ON.colorize for every sample of white [batch, *unit] in `dtype` arithmetic (float64: the reference; float32: numpy's own
    single-precision transform of the same input, the yardstick of `no_further_from_exact`); unbiased std per sample"""
    white = np.asarray(white, dtype=dtype)
    unit = tuple(d for d in white.shape[1:] if d != 1)
    w = white.reshape(white.shape[0], *unit)
    axes = tuple(range(1, w.ndim))
    wstd = w.std(axis=axes, ddof=1, dtype=dtype)
    if exponent == 0.0:
        if energy is None:
            return white
        return white * np.where(wstd < 1e-8, 1.0, energy / wstd).astype(dtype).reshape(-1, *[1] * (white.ndim - 1))
    weights = _weights(unit, float(exponent)).astype(dtype)
    col = np.fft.irfftn(np.fft.rfftn(w, axes=axes) * weights, s=unit, axes=axes).astype(dtype, copy=False)
    cstd = col.std(axis=axes, ddof=1, dtype=dtype)
    scale = np.where(cstd > 1e-8, (wstd if energy is None else dtype(energy)) / cstd, 1.0).astype(dtype)
    return (col * scale.reshape(-1, *[1] * (w.ndim - 1))).reshape(white.shape)


def colorize64(white, exponent: float, energy) -> np.ndarray:
    return colorize_np(white.numpy() if isinstance(white, torch.Tensor) else white, exponent, energy, np.float64)


def sample_errors(got: np.ndarray, exact: np.ndarray) -> np.ndarray:
    "per sample: the relative inf-norm error of got [batch, ...] against exact"
    b = exact.shape[0]
    g, e = np.asarray(got, dtype=np.float64).reshape(b, -1), exact.reshape(b, -1)
    return np.abs(g - e).max(axis=1) / np.abs(e).max(axis=1)
