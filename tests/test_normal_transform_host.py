"""The helpers tests/test_normal_transform_gpu.py rests on, checked without a GPU: the torch restatement of Philox against the oracle and
Random123, the uniform against the oracle's, the word sets against their stated sizes -- and the factor checks themselves, which must pass
float64 parts rounded to fp32 and flag every planted defect."""

import math
import os
import re

import numpy as np
import pytest
import torch

import normal_cases as NC
from conftest import ROOT
from skr_oracle import noise as ON

FIRST_BLOCKS = (0, 2**32 - 2**11, 2**63, 2**64 - 2**11)  # the carry into the counter's high word and the wrap-around, inside 2^12 blocks
SEEDS = (0, 1, 2**40 + 7, 2**64 - 3)
STREAMS = (0, 5 * 256 + 255, 2**32 + 7, 2**63, 2**64 - 1)


def oracle_philox(seed: int, stream: int, first: int, n: int) -> np.ndarray:
    blocks = (np.arange(n, dtype=np.uint64) + np.uint64(first)).astype(np.uint64)  # wraps mod 2^64
    ctr = np.stack([(blocks & np.uint64(0xFFFFFFFF)).astype(np.uint32), (blocks >> np.uint64(32)).astype(np.uint32),
                    np.full(n, stream & 0xFFFFFFFF, np.uint32), np.full(n, stream >> 32, np.uint32)], -1)  # fmt: skip
    return ON.philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))


@pytest.mark.parametrize("first", FIRST_BLOCKS)
def test_philox_words_match_the_oracle_at_the_edges(first):
    with np.errstate(over="ignore"):
        for seed in SEEDS:
            for stream in STREAMS:
                assert np.array_equal(NC.philox_words(seed, stream, first, 1 << 12).numpy(), oracle_philox(seed, stream, first, 1 << 12).astype(np.int64)), (seed, stream)


def test_philox_words_reproduce_random123():
    for (seed, stream, first), want in NC.PHILOX_KATS:
        assert NC.philox_words(seed, stream, first, 1)[0].tolist() == list(want)


def oracle_uniform(words: torch.Tensor) -> np.ndarray:
    "the u of oracle noise.py::box_muller"
    x = words.numpy().astype(np.uint32).astype(np.float32) * ON.TWO_POW_M32 + np.float32(2.0**-33)
    return np.minimum(x, np.float32(1.0))


def test_uniform_and_factors_are_the_oracles():
    "`uniform` is the oracle's u, and `oracle_parts` multiplies out to oracle box_muller bit for bit, on random and on rounding words"
    for words in (NC.random_words(1 << 20, 11), NC.rounding_words()):
        assert np.array_equal(NC.uniform(words).numpy(), oracle_uniform(words))
        r, c, s = (t.numpy() for t in NC.oracle_parts(words))
        quad = words.numpy().astype(np.uint32)[: words.numel() // 4 * 4].reshape(-1, 4)
        z = ON.box_muller(quad).reshape(-1)
        i = np.arange(z.size)
        radius, angle = r[(i // 2) * 2], np.where(i % 2 == 0, c[i | 1], s[i | 1])  # lanes (0, 1) and (2, 3): radius of the even word, angle of the odd
        assert np.array_equal((radius * angle).view(np.uint32), z.view(np.uint32))
    top = NC.uniform(torch.arange(0xFFFFFF00, 1 << 32, dtype=torch.int64))
    assert (top[:128] == np.float32(0.99999994)).all() and (top[128:] == 1).all()  # 1.0 only through conversion rounding
    assert NC.uniform(torch.tensor([0])).item() == 2.0**-33 and NC.R_MAX == pytest.approx(math.sqrt(-2 * math.log(2.0**-33)), rel=1e-15)


def test_representative_words_reach_every_uniform():
    "83,886,080 ascending words, 79,691,776 distinct uniforms from 2^-33 to 0.99999994; a seeded 2^20 random words all land inside that set"
    probe = NC.uniform(NC.random_words(1 << 20, 12))
    probe = probe[probe < 1]  # 128 of 2^32 words reach 1.0, through conversion rounding alone
    found = torch.zeros_like(probe, dtype=torch.bool)
    count = distinct = 0
    last_word, last_u, lo, hi = -1, None, None, None
    for words in NC.representative_words():
        assert words.numel() == NC.CHUNK and words[0] > last_word and (words[1:] > words[:-1]).all() and words[-1] < 1 << 32
        assert torch.equal(NC.representative_of(words), words)
        u = NC.uniform(words)
        assert (u[1:] >= u[:-1]).all()
        distinct += int((u[1:] != u[:-1]).sum()) + (1 if last_u is None or u[0] != last_u else 0)
        found |= u[torch.searchsorted(u, probe).clamp_max(u.numel() - 1)] == probe
        count, last_word, last_u = count + words.numel(), words[-1], u[-1]
        lo, hi = (u[0].item() if lo is None else lo), u[-1].item()
    assert count == NC.N_REPRESENTATIVE and distinct == NC.N_UNIFORMS
    assert lo == 2.0**-33 and hi == float(np.float32(0.99999994)) and found.all()
    r = NC.rounding_words()
    assert r.numel() == 256 + 8 * 3 * (1 << 16) and r.min() >= 0 and r.max() == 0xFFFFFFFF
    # all of them need rounding but 0xFFFFFF00 and, at k = 1, the neighbours (m << 1) and (m << 1) + 2 of the tie
    assert int((NC.representative_of(r) != r).sum()) == 255 + (1 + 3 * 7) * (1 << 16)


def test_recorded_margins_are_the_profiles():
    "the constants the GPU test holds the device to are the ones tools/normal_margins.py wrote down"
    text = open(os.path.join(ROOT, "profiles", "normal_transform.txt")).read()
    spec = text.split("fp32 specification against float64:")[1].split("device")[0]
    for k, v in NC.ORACLE.items():
        assert float(re.search(rf"^\s+{k}\s+(\S+)", spec, flags=re.M).group(1)) == pytest.approx(v, rel=1e-6), k
    assert NC.ORACLE["composed"] == pytest.approx(NC.composed_bound(NC.ORACLE["E_r"], NC.ORACLE["E_c"], NC.ORACLE["E_s"]), rel=1e-6)


# ---- planted defects ----------------------------------------------------------------------------------------------------------
def sparse_chunks():
    "every 61st representative word, and both ends of the range whole: the checks, not the coverage, are under test here"
    for words in NC.representative_words():
        yield torch.cat([words[:4096], words[4096:-65536:61], words[-65536:]])


def rounded_exact(u: torch.Tensor):
    return tuple(t.float() for t in NC.exact_parts(u))


def truncated(words: torch.Tensor) -> torch.Tensor:
    f = words.to(torch.float32)
    return torch.where(f.to(torch.int64) > words, torch.nextafter(f, torch.zeros_like(f)), f)


def _log2_off(sign: float):
    def parts(words):
        u = NC.uniform(words)
        _, c, s = rounded_exact(u)
        return torch.sqrt((-2 * math.log(2) * (torch.log2(u.double()) + sign * 2.0**-24)).clamp_min(0)).float(), c, s

    return parts


def _scaled_trig(words):
    u = NC.uniform(words)
    th = (u * np.float32(2 * math.pi)).double()  # 2 pi u rounded to fp32
    return rounded_exact(u)[0], (1.5 * torch.cos(th)).float(), (1.5 * torch.sin(th)).float()


# name -> (the defective factors, the check that has to catch it)
DEFECTS = {
    "log2 2^-24 high": (_log2_off(+1.0), "rel_r:"),
    "log2 2^-24 low": (_log2_off(-1.0), "rel_r:"),
    "cos / sin of the fp32 angle, scaled by 1.5": (_scaled_trig, "|cos| > 1"),
    "conversion by truncation": (lambda words: rounded_exact(truncated(words) * 2.0**-32 + 2.0**-33), "rounding word differs"),
    "u clamped to 1 - 2^-24": (lambda words: rounded_exact(NC.uniform(words).clamp_max(1 - 2.0**-24)), "r != 0 at u = 1"),
}


def verdict(parts_of) -> list[str]:
    rep = NC.factor_report(parts_of, sparse_chunks(), NC.rounding_words())
    return rep["violations"] + NC.bar_violations(rep, NC.ORACLE)


def test_checks_pass_the_float64_parts_rounded_to_fp32():
    assert verdict(lambda words: rounded_exact(NC.uniform(words))) == []


@pytest.mark.parametrize("name", list(DEFECTS))
def test_checks_flag_planted_defect(name):
    parts_of, caught_by = DEFECTS[name]
    found = verdict(parts_of)
    assert any(caught_by in line for line in found), (name, found)
