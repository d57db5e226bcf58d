"""Every axis length the own any-length transforms (csrc/skr_fft_own.hip) promise, one axis at a time, against float64.

skr_colorize on a caller's white noise never takes the plane kernels: every axis goes through skr_fft_own.hip, and the input is known
exactly, so the float64 reference (tests/fft_lengths.py::colorize64, numpy) needs no Philox.  Every length 2 .. 4096 runs in four roles
-- the only axis (n,), the last of two (3, n), the outer of two (n, 4), the middle of three (3, n, 4) -- and every even length up to
8192 as a last axis.  For each length exactly one of two things holds, by the documented rule (fft_lengths._own_length):

  accepted  SKR_OK; per sample the relative inf-norm error against float64 is below the generator bar 1e-5 (or, failing that, no
            further from float64 than 3 x numpy's float32 transform of the same input: test_noise_gpu.no_further_from_exact); the
            output is finite and fully written; out, spec_c64, white_f32 and partials_f64 are views of a guard-banded arena
            (tests/arena.py) of exactly the header's sizes and the bands stay clean; one own transform ran and hipFFT did not
  refused   SKR_ERR_UNSUPPORTED before anything is written: out, spec_c64 and partials_f64 keep the arena's poison, white_f32 the
            caller's values bit for bit, no counter moves

In that sweep the line counts are tiny, so a tile never fills; test_full_tiles runs the shortest and the longest length of every direct
radix combination and every Bluestein size up to 2048 points (a tile holds 4096: two lines or more) with enough lines for the full
tile, a ragged last one and an unpaired real line.  A fault in one spectral bin moves the output by about 1 / sqrt(N) of its scale -- 4e-3 at 65536 points, more below -- so
a wrong table entry, twiddle or join term cannot hide under 1e-5.

Every Bluestein length is run once into plain buffers first: its tables are allocated at first use and kept for the life of the
process, about 51 MB of device memory over all 1 845 lengths.  Measured errors: profiles/fft_lengths.txt."""

import ctypes
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest
import table_cases as TC
import torch
from arena import Arena, untouched
from conftest import note_margin
from test_noise_gpu import no_further_from_exact

import fft_lengths as FL
from skrample_amd import _hip
from skrample_amd.pytorch import noise as PN

pytestmark = pytest.mark.gpu

BAR = FL.BAR
BLOCKS = [(lo, min(lo + 255, 4096)) for lo in range(2, 4097, 256)]  # 16 blocks of 256 consecutive lengths (the last: 255)
LONG_BLOCKS = [(lo, lo + 510) for lo in range(4098, 8193, 512)]  # 8 blocks of 256 consecutive EVEN lengths
ROLE_TOTALS = {"only": (2934, 1161), "last": (2934, 1161), "outer": (2102, 1993), "middle": (2102, 1993)}  # (accepted, refused) of 4095
LONG_TOTALS = (1793, 255)
_seen: dict = {}  # role -> {block: (accepted, refused)} of this process


@pytest.fixture(scope="module")
def gpu():
    lib = _hip.load()
    dev = torch.device("cuda:0")
    assert lib.skr_set_tuning(b"hipfft", 0) == 0
    yield SimpleNamespace(lib=lib, dev=dev, small=Arena(dev, capacity_bytes=4 << 20), arenas={})
    assert lib.skr_set_tuning(b"hipfft", -1) == 0


def big_arena(gpu) -> Arena:
    if "big" not in gpu.arenas:
        gpu.arenas["big"] = Arena(gpu.dev, capacity_bytes=80 << 20)
    return gpu.arenas["big"]


def stats(gpu) -> tuple:
    return tuple(gpu.lib.skr_stat(k) for k in (b"own_fft_execs", b"hipfft_plans", b"hipfft_execs"))


def colorize(gpu, out, spec, work, partials, batch, dims, exponent, energy) -> int:
    return gpu.lib.skr_colorize(out.data_ptr(), _hip.F32, spec.data_ptr(), work.data_ptr(), partials.data_ptr(), batch, len(dims), (ctypes.c_int32 * len(dims))(*dims),
                                float(exponent), 0 if energy is None else 1, 0.0 if energy is None else float(energy), _hip.current_stream_ptr(gpu.dev))  # fmt: skip


def held(got: np.ndarray, white: torch.Tensor, exponent, energy, family: str, klass: str) -> None:
    "per sample: below the bar against float64 -- or no further from it than 3 x numpy's float32 transform of the same input; every value recorded"
    exact = FL.colorize64(white, exponent, energy)
    errs = FL.sample_errors(got, exact)
    for e in errs:
        note_margin(family, f"device vs float64, {klass}", float(e), BAR)
    if not (errs < BAR).all():
        low = FL.colorize_np(white.numpy(), exponent, energy, np.float32)
        for s in np.nonzero(~(errs < BAR))[0]:
            assert no_further_from_exact(torch.from_numpy(got[s]), torch.from_numpy(low[s]), torch.from_numpy(exact[s]), slack=3.0), (family, klass, tuple(white.shape), s, errs)


def run_length(gpu, arena: Arena, family: str, role: str, dims: tuple, batch: int, n: int, accepted: bool, klass: tuple, warm: bool = False):
    """one skr_colorize call on the axis length n inside `dims`, into guard-banded views of exactly the header's sizes; returns the fp32 output"""
    unit = math.prod(dims)
    half = unit // dims[-1] * (dims[-1] // 2 + 1)
    exponent, energy = FL.exponent_of(n), FL.energy_of(n)
    white = FL.white_input(role, dims, batch)
    white_dev = white.reshape(-1).to(gpu.dev)
    if accepted and (warm or klass[0] != "direct"):  # tables at first use: once eagerly into plain buffers
        plain = (torch.empty(batch * unit, dtype=torch.float32, device=gpu.dev), torch.empty(batch * half, dtype=torch.complex64, device=gpu.dev), white_dev.clone(),
                 torch.empty(4 * batch * 256, dtype=torch.float64, device=gpu.dev))  # fmt: skip
        assert colorize(gpu, *plain, batch, dims, exponent, energy) == 0, (dims, "plain buffers")
    arena.reset()
    out = arena.take("out", batch * unit, torch.float32)
    spec = arena.take("spec_c64", batch * half, torch.complex64)
    work = arena.take("white_f32", batch * unit, torch.float32)
    partials = arena.take("partials_f64", 4 * batch * 256, torch.float64)
    work.copy_(white_dev)
    before = stats(gpu)
    status = colorize(gpu, out, spec, work, partials, batch, dims, exponent, energy)
    torch.cuda.synchronize()
    after = stats(gpu)
    arena.check()
    if not accepted:
        assert status == _hip.SKR_ERR_UNSUPPORTED, (dims, status)
        assert untouched(out) and untouched(spec) and untouched(partials), (dims, "a refused call wrote to an output or a workspace")
        assert torch.equal(work, white_dev), (dims, "a refused call changed the caller's white noise")
        assert after == before, (dims, before, after)
        return None
    assert status == 0, (dims, status, gpu.lib.skr_strerror(status).decode())
    arena.assert_written("out")
    assert torch.isfinite(out).all(), dims
    assert after == (before[0] + 1, before[1], before[2]), (dims, before, after)
    got = out.cpu().numpy().reshape(batch, *dims)
    held(got, white, exponent, energy, family, FL.class_name(klass))
    return got


# ---- every length 2 .. 4096 in four roles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", BLOCKS, ids=lambda b: f"{b[0]}-{b[1]}")
@pytest.mark.parametrize("role", FL.ROLES)
def test_every_length(role, block, gpu):
    counts = [0, 0]
    for n in range(block[0], block[1] + 1):
        last = role in ("only", "last")
        accepted = FL._own_length(n, last)
        run_length(gpu, gpu.small, f"own fft {role}", role, FL.role_dims(role, n), 2, n, accepted, FL.classify(n, last))
        counts[0 if accepted else 1] += 1
    assert sum(counts) == block[1] - block[0] + 1
    _seen.setdefault(role, {})[block] = tuple(counts)


def test_totals_of_every_role():
    """the documented rule accepts and refuses as many lengths per role as were counted from the header (tests/test_fft_lengths_host.py).
    What the DEVICE accepted and refused is compared block by block for the blocks that ran in this process, and summed only when all 16
    of a role did: under a -k selection, or with the tests spread over worker processes, this test checks the predicate's counts alone."""
    for role, (accepted, refused) in ROLE_TOTALS.items():
        want = [sum(FL.role_accepts(role, n) for n in range(lo, hi + 1)) for lo, hi in BLOCKS]
        assert sum(want) == accepted and 4095 - sum(want) == refused, role
        ran = _seen.get(role, {})
        for (lo, hi), w in zip(BLOCKS, want):
            assert (lo, hi) not in ran or ran[(lo, hi)] == (w, hi - lo + 1 - w), (role, lo)
        if len(ran) == len(BLOCKS):
            assert (sum(a for a, _ in ran.values()), sum(r for _, r in ran.values())) == (accepted, refused), role


# ---- full tiles --------------------------------------------------------------------------------------------------------------------------
def full_tile_lengths() -> list:
    """the shortest and the longest length of every direct radix multiset and every Bluestein (m, r) class whose transform has at most
    FFT_MAX_TILE / 2 = 2048 points: those whose full tile holds two lines or more"""
    classes: dict = {}
    for n in range(2, 2049):
        c = FL.classify(n)
        if FL.transform_size(c) <= 2048:
            assert FL.full_tile(FL.transform_size(c)) >= 2
            classes.setdefault((c[0], c[2]) if c[0] == "direct" else c, []).append(n)
    return sorted({n for ns in classes.values() for n in (ns[0], ns[-1])})


def lines_for_full_tile(m: int) -> int:
    "the fewest lines for which the tile is full AND a second, ragged tile follows"
    L = FL.full_tile(m)
    need = L + 1  # (a transform so short that half a tile would leave threads without two points: the tile is never halved)
    if FL.tile_lines(m, need) != L:
        need = 511 * L + 1  # 512 blocks
        assert FL.tile_lines(m, need - 1) < L
    assert L >= 2 and FL.tile_lines(m, need) == L and need % L
    return need


def full_tile_dims(role: str, n: int) -> tuple:
    """role last: K real lines of n points, K the smallest odd count whose (K + 1) / 2 pairs fill the tile -- as (K, n) while K is itself a
    length the outer pass takes, else split (K1, K2, n) into two odd short lengths (their product: the line count).
    role outer: (n, K), the K / 2 + 1 spectral columns one more than fill the tile; K the next length admissible as a last axis."""
    m = FL.transform_size(FL.classify(n))
    L, need = FL.full_tile(m), lines_for_full_tile(m)
    if role == "last":
        K = max(2 * need - 1, 3)
        if FL._short_length(K):
            return (K, n)
        k1 = 3
        while -(-K // k1) > 2047:
            k1 += 2
        k2 = -(-K // k1) | 1
        while ((k1 * k2 + 1) // 2) % L == 0:
            k2 += 2
        assert k2 <= 2047 and FL.tile_lines(m, (k1 * k2 + 1) // 2) == L
        return (k1, k2, n)
    K = 2 * (need - 1) + 1
    while not FL._own_length(K, last=True) or (K // 2 + 1) % L == 0 or K // 2 + 1 < need:
        K += 1
    assert FL.tile_lines(m, K // 2 + 1) == L
    return (n, K)


FULL_TILE_GROUPS = 12  # (a full tile of a long transform needs some 4 M elements: a dozen lengths and two to three seconds a group)


@pytest.mark.parametrize("group", range(FULL_TILE_GROUPS))
def test_full_tiles(group, gpu):
    lengths = full_tile_lengths()
    assert len(lengths) == 138  # (some classes hold one length only)
    for n in lengths[group::FULL_TILE_GROUPS]:
        klass = FL.classify(n)
        for role in ("last", "outer"):
            dims = full_tile_dims(role, n)
            assert math.prod(dims) <= 5 << 20, dims
            assert run_length(gpu, big_arena(gpu), "own fft full tile", f"full tile {role}", dims, 1, n, True, klass, warm=True) is not None


# ---- long last axes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", LONG_BLOCKS, ids=lambda b: f"{b[0]}-{b[1]}")
def test_every_even_length_as_a_long_last_axis(block, gpu):
    counts = [0, 0]
    for n in range(block[0], block[1] + 1, 2):
        klass = FL.classify(n, last=True)
        assert klass[0] in ("long", "refused")
        run_length(gpu, gpu.small, "own fft long", "long", (2, n), 2, n, klass[0] == "long", klass)
        counts[0 if klass[0] == "long" else 1] += 1
    assert sum(counts) == 256
    _seen.setdefault("long", {})[block] = tuple(counts)


def test_totals_of_the_long_last_axes():
    "as test_totals_of_every_role: the device's own total is summed only when all eight blocks ran in this process"
    want = [sum(FL._own_length(n, last=True) for n in range(lo, hi + 1, 2)) for lo, hi in LONG_BLOCKS]
    assert (sum(want), 2048 - sum(want)) == LONG_TOTALS
    ran = _seen.get("long", {})
    for (lo, hi), w in zip(LONG_BLOCKS, want):
        assert (lo, hi) not in ran or ran[(lo, hi)] == (w, 256 - w), lo
    if len(ran) == len(LONG_BLOCKS):
        assert (sum(a for a, _ in ran.values()), sum(r for _, r in ran.values())) == LONG_TOTALS
    assert not any(FL._own_length(2 * p, last=True) for p in (2053, 4093, 4099))  # 2 x prime: no split


def split_kinds() -> dict:
    """the first even length beyond 4096 of each kind of split: both factors direct, one of them, neither -- among the lengths whose split
    does not depend on how "direct" is read (fft_lengths._loosely_direct: the scoring in the source reads it more loosely than the header)"""
    found: dict = {}
    for n in range(4098, 8193, 2):
        c = FL.classify(n, last=True)
        if c[0] == "long" and FL.long_split(n, loose=True) == c[1:] and all((FL.classify(f)[0] == "direct") == FL._loosely_direct(f) for f in c[1:]):
            found.setdefault(sum(FL.classify(f)[0] == "bluestein" for f in c[1:]), n)
    return found


def test_long_splits_of_every_kind_and_65536(gpu):
    kinds = split_kinds()
    assert sorted(kinds) == [0, 1, 2], kinds
    for bluesteins, n in sorted(kinds.items()):
        assert run_length(gpu, gpu.small, "own fft long", "long", (2, n), 2, n, True, FL.classify(n, last=True)) is not None, (bluesteins, n)
    assert FL.classify(65536, last=True) == ("long", 128, 256)
    assert run_length(gpu, gpu.small, "own fft long", "only", (65536,), 2, 65536, True, ("long", 128, 256)) is not None


# ---- the product's paths -----------------------------------------------------------------------------------------------------------------
def product_sample() -> list:
    rng = random.Random(4096)
    return [(role, n) for role in FL.ROLES for n in sorted(rng.sample([n for n in range(2, 4097) if FL.role_accepts(role, n)], 12))]


def generate_sample(role: str) -> list:
    """12 accepted lengths of a role of rank 1 or 2 whose unit Colored.generate draws on the own transforms: the product sends 2-D
    powers of two and 2-D units with an even height and a width that is a multiple of 4 to the plane kernels first (in role outer, (n, 4),
    that leaves the odd n), and a 3-D unit may take them too -- role middle has no draw here.  The test asserts the counter."""
    if role == "middle":
        return []
    own = [n for n in range(2, 4097) if FL.role_accepts(role, n) and not PN.Colored._axes(FL.role_dims(role, n))[1] and not PN.Colored._mixed_radix_candidate(list(FL.role_dims(role, n)))]
    return sorted(random.Random(8192 + FL.ROLES.index(role)).sample(own, 12))


@pytest.mark.parametrize("role", FL.ROLES)
def test_the_products_paths(role, gpu):
    """colorize_noise has the ABI call's bits (fp32) and rounds them once (bf16) at 12 sampled lengths; Colored.generate meets the bar on
    skr_noise_random's draw at 12 lengths it draws on the own transforms (generate_sample)"""
    sample = [n for r, n in product_sample() if r == role]
    assert len(sample) == 12
    for n in sample:
        dims = FL.role_dims(role, n)
        klass = FL.classify(n, role in ("only", "last"))
        exponent, energy = FL.exponent_of(n), FL.energy_of(n)
        direct = run_length(gpu, gpu.small, f"own fft {role}", role, dims, 1, n, True, klass)
        white = FL.white_input(role, dims, 1)[0].to(gpu.dev)
        got = PN.Colored.colorize_noise(white, exponent, energy)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), direct[0].view(np.uint32)), dims
        white16 = white.bfloat16()
        assert torch.equal(PN.Colored.colorize_noise(white16, exponent, energy), PN.Colored.colorize_noise(white16.float(), exponent, energy).bfloat16()), dims
    for n in generate_sample(role):
        dims = FL.role_dims(role, n)
        klass = FL.classify(n, role in ("only", "last"))
        exponent, energy = FL.exponent_of(n), FL.energy_of(n)
        seeds = [1000 + n, 2**40 + n]
        before = stats(gpu)
        g = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, dims, seeds, props=PN.ColoredProps(color_start=exponent, energy=energy), dtype=torch.float32)
        drawn = g.generate(None)
        assert stats(gpu) == (before[0] + 1, before[1], before[2]), (dims, "the draw did not run on the own transforms")
        draw = torch.empty(2 * math.prod(dims), dtype=torch.float32, device=gpu.dev)
        seeds_dev = TC.seeds_tensor(seeds).to(gpu.dev)
        assert gpu.lib.skr_noise_random(draw.data_ptr(), _hip.F32, seeds_dev.data_ptr(), 0, 2, math.prod(dims), _hip.current_stream_ptr(gpu.dev)) == 0
        torch.cuda.synchronize()
        assert torch.isfinite(drawn).all()
        held(drawn.cpu().numpy().reshape(2, *dims), draw.cpu().reshape(2, *dims), exponent, energy, f"own fft {role}", "Colored.generate, " + FL.class_name(klass))
