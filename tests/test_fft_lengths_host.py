"""tests/fft_lengths.py against the oracle and against the documented length rule: the float64 reference of the length sweep
(tests/test_fft_lengths_gpu.py) is the oracle's colorize, and the classification counts what the header of csrc/skr_fft_own.hip promises."""

import numpy as np
import pytest
import torch
from skr_oracle import noise as ON

import fft_lengths as FL

# (few and small: the sweep itself never calls torch's CPU FFT, whose float64 transforms have crashed the interpreter in long loops over lengths)
SHAPES = [((5,), None), ((444,), 2.5), ((2050,), None), ((3, 17), None), ((3, 130), 2.5), ((97, 4), None), ((250, 4), 2.5), ((1, 66, 1), None),
          ((3, 19, 4), None), ((3, 26, 4), 2.5), ((2, 30, 40), None), ((4, 1, 12), 0.5)]  # fmt: skip


@pytest.mark.parametrize(("unit", "energy"), SHAPES, ids=[f"{u}-{e}" for u, e in SHAPES])
def test_colorize64_is_the_oracles_colorize(unit, energy):
    "two samples a call (the second shifted: a live DC bin), each against ON.colorize of that sample alone, float64, within 1e-12 of the output's scale"
    white = FL.white_input("host", unit).double()
    exponent = FL.EXPONENTS[len(unit) % 3] if unit != (5,) else 1.7
    got = FL.colorize64(white, exponent, energy)
    assert got.dtype == np.float64 and got.shape == tuple(white.shape)
    for s in range(white.shape[0]):
        ref = ON.colorize(white[s].clone(), exponent, energy).numpy()
        assert np.abs(got[s] - ref).max() <= 1e-12 * np.abs(ref).max(), (unit, s)
    if energy is not None:
        assert np.allclose(got.reshape(2, -1).std(axis=1, ddof=1), energy, rtol=1e-12)


def test_colorize64_without_an_exponent_rescales_only():
    white = FL.white_input("host", (7, 6)).double()
    assert np.array_equal(FL.colorize64(white, 0.0, None), white.numpy())
    for s, row in enumerate(FL.colorize64(white, 0.0, 2.5)):
        assert np.abs(row - ON.colorize(white[s].clone(), 0.0, 2.5).numpy()).max() <= 1e-12 * np.abs(row).max()


def test_the_single_precision_yardstick_stays_in_single_precision():
    "numpy's float32 transform is what `no_further_from_exact` measures the device against: it must not silently run in float64"
    white = FL.white_input("host", (3, 130)).numpy()
    low, exact = FL.colorize_np(white, 0.25, None, np.float32), FL.colorize64(white, 0.25, None)
    assert low.dtype == np.float32 and np.fft.rfftn(white, axes=(1, 2)).dtype == np.complex64
    err = FL.sample_errors(low, exact)
    assert (err > 0).all() and (err < FL.BAR).all(), err


def test_constants_are_the_sources():
    assert FL.constants() == {"OWN_MAX_M": 4096, "FFT_MAX_TILE": 4096, "FFT_THREADS": 256}


def test_classification_counts_what_the_header_promises():
    lengths = range(2, 4097)
    other = {n: FL.classify(n) for n in lengths}
    last = {n: FL.classify(n, last=True) for n in lengths}
    short = [n for n in lengths if FL._short_length(n)]
    direct = [n for n in lengths if other[n][0] == "direct"]
    bluestein = [n for n in lengths if other[n][0] == "bluestein"]
    assert len(short) == 2102 and sorted(direct + bluestein) == short
    assert len(direct) == 257 and len({other[n][2] for n in direct}) == 55  # (the powers of two are the multiset without a factor)
    assert len(bluestein) == 1845 and len({other[n][1:] for n in bluestein}) == 27
    assert all(last[n] == other[n] for n in short)
    assert sum(last[n][0] == "long" for n in lengths) == 832
    assert sum(last[n][0] == "refused" for n in lengths) == 1161
    assert sum(other[n][0] == "refused" for n in lengths) == 1993
    even = range(4098, 8193, 2)
    assert sum(FL.classify(n, last=True)[0] == "long" for n in even) == 1793 and len(even) == 2048
    assert all(FL.classify(n)[0] == "refused" for n in range(4097, 8193))
    for n in range(2, 8193):  # the classification refuses what the predicates refuse, and nothing else
        assert (FL.classify(n)[0] != "refused") == FL._own_length(n) and (FL.classify(n, last=True)[0] != "refused") == FL._own_length(n, last=True), n
    for role, accepted in (("only", 2934), ("last", 2934), ("outer", 2102), ("middle", 2102)):
        assert sum(FL.role_accepts(role, n) for n in lengths) == accepted, role


def test_classification_of_known_lengths():
    "the header's own examples"
    assert FL.classify(4096) == ("direct", 4096, ()) and FL.classify(2) == ("direct", 2, ())
    assert FL.classify(66) == ("direct", 2, (3, 11)) and FL.classify(1280) == ("direct", 256, (5,)) and FL.classify(720) == ("direct", 16, (3, 3, 5))
    assert FL.classify(3840) == ("direct", 256, (3, 5)) and FL.classify(4004) == ("direct", 4, (7, 11, 13))
    assert FL.classify(1080)[0] == "bluestein" and FL.classify(1500)[0] == "bluestein"  # four odd factors
    assert FL.classify(15)[0] == "bluestein" and FL.classify(3) == ("bluestein", 6, 3)  # odd: no power of two to transform
    assert FL.classify(130 * 3) == ("direct", 2, (3, 5, 13)) and FL.classify(97) == ("bluestein", 256, 1)
    assert FL.classify(161) == ("bluestein", 384, 3)  # 2 n - 1 = 321: 384 instead of 512
    assert FL.classify(641) == ("bluestein", 1536, 3) and FL.classify(1025) == ("bluestein", 2560, 5) and FL.classify(2047) == ("bluestein", 4096, 1)
    assert FL.classify(2050) == ("refused",) and FL.classify(2050, last=True) == ("long", 25, 41)
    assert FL.classify(65536, last=True) == ("long", 128, 256) and FL.classify(8192, last=True) == ("long", 64, 64)
    assert FL.classify(2 * 4099, last=True) == ("refused",) and FL.classify(4097, last=True) == ("refused",)
    assert FL.classify(4160) == ("refused",) and FL.classify(4160, last=True) == ("long", 40, 52)  # 2^6 5 13: direct in form, but beyond 4096


def test_where_the_scorings_reading_of_direct_moves_the_split():
    """own_long_split prefers "direct" factors, but reads the word more loosely than own_axis and the header do (fft_lengths._loosely_direct:
    9, 25, 361 x 3 ...).  Which lengths are accepted does not depend on it; 179 of the 2 625 long last axes up to 8192 get other factors
    than the documented preference would pick (2166: 3 x 361, both through Bluestein, where 19 x 57 is as admissible and squarer).
    The device tests pick their direct x direct / Bluestein examples among the lengths where both readings agree."""
    long = [n for n in range(2050, 8193, 2) if FL.classify(n, last=True)[0] == "long"]
    assert len(long) == 832 + 1793
    assert all((FL.long_split(n) is None) == (FL.long_split(n, loose=True) is None) for n in range(2, 8193, 2))
    moved = [n for n in long if FL.long_split(n) != FL.long_split(n, loose=True)]
    assert len(moved) == 179 and moved[:3] == [2052, 2166, 2244]
    assert FL.long_split(2166) == (19, 57) and FL.long_split(2166, loose=True) == (3, 361)
    assert FL._loosely_direct(9) and FL._loosely_direct(3003) and FL.direct_form(9) is None and FL.direct_form(3003) is None


def test_tile_lines_follows_the_sources_rule():
    assert FL.full_tile(1024) == 4 and FL.full_tile(2048) == 2 and FL.full_tile(4096) == 1 and FL.full_tile(320) == 8 and FL.full_tile(2) == 256
    assert FL.tile_lines(1024, 4 * 511) == 2 and FL.tile_lines(1024, 4 * 511 + 1) == 4  # full from 512 blocks on; 2 x 1022 blocks below
    assert FL.tile_lines(1024, 3) == 1 and FL.tile_lines(256, 3) == 2 and FL.tile_lines(256, 16 * 511 + 1) == 16
    assert FL.tile_lines(320, 8 * 511) == 4 and FL.tile_lines(320, 8 * 511 + 1) == 8 and FL.tile_lines(320, 3) == 2  # (one line of 320 points is fewer than two a thread)
    assert FL.tile_lines(2, 1) == 256  # half of it would leave threads without two points: never halved
    for m in (6, 10, 16, 48, 130, 320, 1024, 2560, 4096):
        for lines in (1, 2, 5, 511, 512, 4096, 1 << 20):
            L = FL.tile_lines(m, lines)
            assert L & (L - 1) == 0 and 1 <= L <= FL.full_tile(m) and (L == 1 or L * m <= 4096)
