"""Word sets, float64 references and checks for the Philox-to-normal transform (skrample_amd/csrc/skr_philox.h).

z0 = r(u0) * cos(2 pi u1), z1 = r(u0) * sin(2 pi u1), r(u) = sqrt(-2 ln u), u = fl32(fl32(x) * 2^-32 + 2^-33): every factor depends on ONE
fp32 uniform, and the 2^32 words reach only ~8e7 distinct uniforms -- so each factor can be checked on EVERY reachable input, which bounds
the error of every one of the 2^64 pairs (`composed_bound`).  Everything here is plain torch and runs on any device: the GPU test feeds
the checks with the device's factors, the host test with float64 parts rounded to fp32 and with planted defects.

Words travel as int64 tensors holding 0 .. 2^32 - 1."""

from __future__ import annotations

import math
import os
import sys
from typing import Callable, Iterator

import numpy as np
import torch

CHUNK = 1 << 24
N_REPRESENTATIVE = 83_886_080  # 2^24 + 8 * 2^23
N_UNIFORMS = 79_691_776  # distinct fp32 uniforms those words reach: 2^-33 .. 0.99999994 (1.0 only through conversion rounding)
R_MAX = math.sqrt(66 * math.log(2))  # r(2^-33) = sqrt(-2 ln 2^-33) = 6.7638..., the largest radius
ULP = 2.0**-24  # the unit the relative error of r is stated in
_MASK = 0xFFFFFFFF
SLACK = 1.5  # tests/test_noise_gpu.py::no_further_from_exact's slack
# The fp32 specification's own distance from float64 over representative_words() and rounding_words(), as tools/normal_margins.py
# measured it: profiles/normal_transform.txt (tests/test_normal_transform_host.py holds these constants to that file).
ORACLE = {"E_r": 3.955093e-07, "E_c": 3.797082e-07, "E_s": 4.163200e-07, "rel_r": 2.870228, "composed": 3.614523e-06}


# ---- word sets -------------------------------------------------------------------------------------------------------------
def representative_words(device="cpu") -> Iterator[torch.Tensor]:
    """the 83,886,080 words fp32 represents exactly -- every x < 2^24, then m * 2^k for 2^23 <= m < 2^24, k = 1..8 -- ascending, in
    chunks of 2^24"""
    yield torch.arange(CHUNK, dtype=torch.int64, device=device)
    m = torch.arange(1 << 23, 1 << 24, dtype=torch.int64, device=device)
    for k in (1, 3, 5, 7):
        yield torch.cat([m << k, m << (k + 1)])


def rounding_words(device="cpu") -> torch.Tensor:
    """words the uint32 -> fp32 conversion has to round: all of 0xFFFFFF00..0xFFFFFFFF (the top 128 round to 2^32, i.e. u = 1), and for
    k = 1..8 and 2^16 seeded m the tie (m << k) + 2^(k-1) with the word below and the word above it"""
    gen = torch.Generator().manual_seed(0x5EED)
    out = [torch.arange(0xFFFFFF00, 1 << 32, dtype=torch.int64)]
    for k in range(1, 9):
        m = torch.randint(1 << 23, 1 << 24, (1 << 16,), generator=gen, dtype=torch.int64)
        half = 1 << (k - 1)
        out += [(m << k) + half - 1, (m << k) + half, (m << k) + half + 1]
    return torch.cat(out).to(device)


def random_words(n: int, seed: int, device="cpu") -> torch.Tensor:
    return torch.randint(0, 1 << 32, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(device)


def representative_of(words: torch.Tensor) -> torch.Tensor:
    "the exactly representable word round-to-nearest-even selects (2^32, which is no word, for the top 128)"
    return words.to(torch.float32).to(torch.int64)


def as_u32_bits(words: torch.Tensor) -> torch.Tensor:
    "int64 0 .. 2^32-1 -> int32 with the same low 32 bits"
    return ((words << 32) >> 32).to(torch.int32)


# ---- the specification in float64 ----------------------------------------------------------------------------------------------
def uniform(words: torch.Tensor) -> torch.Tensor:
    "fl32(fl32(x) * 2^-32 + 2^-33): torch's int64 -> float32 rounds to nearest even, the product is exact, the sum rounds once"
    return words.to(torch.float32) * 2.0**-32 + 2.0**-33


def exact_parts(u: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    "float64 (sqrt(-2 ln u), cos 2 pi u, sin 2 pi u) of fp32 uniforms"
    d = u.double()
    th = d * (2 * math.pi)
    return torch.sqrt(-2 * torch.log(d)), torch.cos(th), torch.sin(th)


def composed_bound(e_r: float, e_c: float, e_s: float) -> float:
    """worst |z - exact| over all 2^64 pairs given the factor maxima: |fl(r' c') - r c| <= |r' - r| |c'| + r |c' - c| + |r' c'| 2^-24
    <= E_r + R max(E_c, E_s) + R 2^-24 (second-order terms dropped: they are below 1e-12)"""
    return e_r + R_MAX * max(e_c, e_s) + R_MAX * ULP


def philox_words(seed: int, stream: int, first_block: int, n: int, device="cpu") -> torch.Tensor:
    """[n, 4] words of Philox4x32-10 blocks first_block .. first_block + n - 1 (mod 2^64) of (seed, stream), in int64: a 32x32 product
    wraps mod 2^64, so its low half is `& 0xFFFFFFFF` and its high half `(>> 32) & 0xFFFFFFFF`"""
    assert 0 <= n < 1 << 32
    i = torch.arange(n, dtype=torch.int64, device=device)
    lo = (first_block & _MASK) + i  # < 2^33
    c0, c1 = lo & _MASK, (((first_block >> 32) & _MASK) + (lo >> 32)) & _MASK
    c2, c3 = torch.full_like(i, stream & _MASK), torch.full_like(i, (stream >> 32) & _MASK)
    k0, k1 = seed & _MASK, (seed >> 32) & _MASK
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = ((p1 >> 32) & _MASK) ^ c1 ^ k0, p1 & _MASK, ((p0 >> 32) & _MASK) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + 0x9E3779B9) & _MASK, (k1 + 0xBB67AE85) & _MASK
    return torch.stack([c0, c1, c2, c3], -1)


# Random123's kat_vectors for philox4x32-10 as ((seed, stream, first_block), words): counter = (block lo, block hi, stream lo, stream hi),
# key = (seed lo, seed hi)
PHILOX_KATS = (
    ((0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    (((1 << 64) - 1,) * 3, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x299F31D0A4093822, 0x0370734413198A2E, 0x85A308D3243F6A88), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def oracle_parts(words: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the factors of the fp32 oracle's Box-Muller (oracle noise.py::box_muller, whose products tests/test_normal_transform_host.py holds
    these to bit for bit), fp32 numpy on the host"""
    try:
        from skr_oracle import noise as ON
    except ImportError:  # outside pytest (tools/normal_margins.py) nothing has put the oracle on the path yet
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
        from skr_oracle import noise as ON

    x = words.cpu().numpy().astype(np.uint32).astype(np.float32) * ON.TWO_POW_M32 + np.float32(2.0**-33)
    x = np.minimum(x, np.float32(1.0))
    r = np.sqrt(np.float32(-2.0) * np.log(x)).astype(np.float32)
    th = (ON.TWO_PI * x).astype(np.float32)
    return torch.from_numpy(r), torch.from_numpy(np.cos(th)), torch.from_numpy(np.sin(th))


# ---- the checks, as functions of a factor triple -----------------------------------------------------------------------------
PartsOf = Callable[[torch.Tensor], tuple[torch.Tensor, torch.Tensor, torch.Tensor]]  # words -> fp32 (r(word), cos(word), sin(word))


def factor_report(parts_of: PartsOf, chunks, rounding: torch.Tensor) -> dict:
    """Run `parts_of` over every chunk of words and over the rounding words.  Returns the measured maxima -- E_r, E_c, E_s (absolute,
    against `exact_parts` of `uniform(words)`) and rel_r (relative error of r where r > 0, in units of 2^-24) -- and `violations`, the
    conditions that need no measurement and do not hold (an empty list when all do)."""
    e = {"E_r": 0.0, "E_c": 0.0, "E_s": 0.0, "rel_r": 0.0}
    bad: list[str] = []

    def flag(name: str, mask: torch.Tensor, words: torch.Tensor):
        n = int(mask.sum())
        if n:
            bad.append(f"{name}: {n} words, first 0x{int(words[mask][0]):08x}")

    def one(words: torch.Tensor):
        u = uniform(words)
        xr, xc, xs = exact_parts(u)
        r, c, s = parts_of(words)
        flag("not finite", ~(torch.isfinite(r) & torch.isfinite(c) & torch.isfinite(s)), words)
        flag("r != 0 at u = 1", (u == 1) & (r != 0), words)
        flag("r <= 0 at u < 1", (u < 1) & ~(r > 0), words)
        flag("r above R (1 + 2^-22)", ~(r.double() <= R_MAX * (1 + 2.0**-22)), words)
        flag("|cos| > 1", ~(c.abs() <= 1), words)
        flag("|sin| > 1", ~(s.abs() <= 1), words)
        dr, dc, ds = (r.double() - xr).abs(), (c.double() - xc).abs(), (s.double() - xs).abs()
        m_r, m_c, m_s = dr.max().item(), dc.max().item(), ds.max().item()
        flag("sign of cos", (xc.abs() > m_c) & (torch.signbit(c) != torch.signbit(xc)), words)
        flag("sign of sin", (xs.abs() > m_s) & (torch.signbit(s) != torch.signbit(xs)), words)
        pos = xr > 0
        rel = (torch.where(pos, dr / torch.where(pos, xr, torch.ones_like(xr)), torch.zeros_like(dr)).max() / ULP).item()
        for k, v in (("E_r", m_r), ("E_c", m_c), ("E_s", m_s), ("rel_r", rel)):
            e[k] = max(e[k], v) if v == v else float("nan")
        return r, c, s

    for words in chunks:
        one(words)
    got = one(rounding)
    rep = representative_of(rounding)
    has = rep < (1 << 32)  # the top 128 round to u = 1, which no exactly representable word reaches: the conditions above cover them
    want = parts_of(torch.where(has, rep, torch.zeros_like(rep)))
    differs = torch.zeros_like(has)
    for g, w in zip(got, want):
        differs |= g.view(torch.int32) != w.view(torch.int32)
    flag("rounding word differs from its round-to-nearest-even representative", has & differs, rounding)
    e["composed"] = composed_bound(e["E_r"], e["E_c"], e["E_s"])
    e["violations"] = bad
    return e


def bar_violations(measured: dict, oracle: dict) -> list[str]:
    """the bar: no further from float64 than the fp32 oracle is, x SLACK -- for the composed bound of every z, and for the relative error of r
    (the one that catches a log2 that cancels near u -> 1)"""
    out = []
    for k in ("composed", "rel_r"):
        if not measured[k] <= SLACK * oracle[k]:
            out.append(f"{k}: {measured[k]:.4g} > {SLACK} x {oracle[k]:.4g}")
    return out
