"""No entry of the C ABI stores outside a buffer its caller provides.

Every output and workspace here is a view of one poisoned allocation (tests/arena.py) with 64 KiB of guard band on each side, sized
EXACTLY as include/skrample_hip.h documents; after each call the bands must be untouched, every output fully written and finite, and
the result must meet the bar the entry's own test already uses: the oracle fed the specified Philox draws for the generators (the
helpers and tolerances of tests/test_noise_gpu.py, nothing new), bit equality with the same launch into plain tensors for the
deterministic entries.  A 16-bit or fp64 draw is the fp32 draw rounded once / widened (the output-dtype contract of the header).
Each noise shape is also drawn by the product's own generator, whose workspaces must be at least as large as the banded run's.
Reads past a buffer are out of scope: they cannot be observed without a fault."""

import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import table_cases as TC
import torch
from arena import Arena, untouched
from skr_oracle import noise as ON
from test_noise_gpu import COLORED_TOL, PYRAMID_TOL, TOL, pyramid_reference, rel, spec_normal

from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.pytorch import noise as PN
from skrample_amd.pytorch._philox_host import uniform01
from skrample_amd.rolling import advance_reference

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]
NAMES = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32", torch.float64: "fp64"}
dtype_ids = NAMES.get
SEEDS = (31, 2**40 + 7, 77)  # batch 1 takes the first, batch 3 all of them
WHITE_BAR = 4e-6  # device normal against oracle philox_normal: what test_random_generator asserts


@pytest.fixture(scope="module")
def gpu():
    lib = _hip.load()
    dev = torch.device("cuda:0")
    return SimpleNamespace(lib=lib, dev=dev, arena=Arena(dev, capacity_bytes=96 << 20))


@pytest.fixture
def arena(gpu):
    gpu.arena.reset()
    return gpu.arena


def hs(gpu):
    return _hip.current_stream_ptr(gpu.dev)


def ok(gpu, status: int, what: str) -> None:
    assert status == 0, f"{what}: status {status} ({gpu.lib.skr_strerror(status).decode()})"


def settle(arena: Arena, *outputs: str) -> None:
    "after a call: the bands are untouched, every named output is fully written and finite"
    torch.cuda.synchronize()
    arena.check()
    for name in outputs:
        arena.assert_written(name)
        assert torch.isfinite(arena.view(name).double()).all(), name


_seed_vectors: dict = {}


def seeds_dev(gpu, values) -> torch.Tensor:
    "the device seed vector of these values; kept for the life of the module, so that a call may take its pointer from a temporary"
    key = tuple(values)
    if key not in _seed_vectors:
        _seed_vectors[key] = TC.seeds_tensor(list(values)).to(gpu.dev)
    return _seed_vectors[key]


def i64s(values):
    return (ctypes.c_int64 * len(values))(*values)


def i32s(values):
    return (ctypes.c_int32 * len(values))(*values)


@functools.lru_cache(maxsize=None)
def normal(seed: int, stream: int, shape: tuple) -> torch.Tensor:
    return spec_normal(seed, stream, shape)


def same_draw(got: torch.Tensor, draw32: torch.Tensor) -> bool:
    "the output-dtype contract: an fp32 draw stored as `got.dtype` is the fp32 value rounded once (widened, for float64)"
    return torch.equal(got.cpu().reshape(-1), draw32.cpu().reshape(-1).to(got.dtype))


def product_holds(kind, unit, seeds, props, given, step=None) -> None:
    """The product's own generator draws this shape, and every workspace it keeps is at least as large as the banded run was given
    (`given`: (dtype, numel) per workspace).  What that shows: the sizes that do not depend on a slot count (scratch, spectrum, level
    table, cache, the LDS kernels' partials) are the header's.  Where `given` is computed from a copy of the product's own slot formula
    (python_slots, python_colored_slots) the comparison only pins that copy to the product; the containment of that slot count is what
    the banded run at it showed.  Random and Offset keep no workspace: `given` is empty and the call shows only that they draw."""
    g = PN.BatchTensorNoise.from_batch_inputs(kind, tuple(unit), list(seeds), props=props, dtype=torch.float32)
    out = g.generate(step)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    seen, pools = set(), {}
    for t in g.workspace_tensors()[1:]:  # (the first is the seed vector: read only)
        if t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            pools.setdefault(t.dtype, []).append(t.numel())
    for dtype, numel in sorted(given, key=lambda x: -x[1]):
        fits = [s for s in pools.get(dtype, []) if s >= numel]
        assert fits, f"{kind.__name__}{tuple(unit)}: no {dtype} workspace of at least {numel} elements among {pools}"
        pools[dtype].remove(min(fits))


def test_the_arena_catches_a_planted_store_on_the_device(gpu, arena):
    "tests/test_arena_host.py on the device the kernels write to: one element behind a view, one in front, one element left unwritten"
    out = arena.take("out", 2048 + 3, torch.bfloat16, offset_elems=1)
    slots = arena.take("slots", 4, torch.float64)
    out.zero_()
    slots.zero_()
    settle(arena, "out", "slots")
    behind = (slots.data_ptr() - arena.buf.data_ptr()) + 4 * 8
    arena.buf[behind : behind + 8] = 0  # slot `n_slots` of a buffer that has n_slots slots
    with pytest.raises(AssertionError, match=r"slots \(4 x torch.float64\), band after: 8 byte\(s\) changed, bytes 0 .. 7"):
        arena.check()
    arena.buf[behind : behind + 8] = 0xFF
    front = out.data_ptr() - arena.buf.data_ptr() - 2
    arena.buf[front : front + 2] = 0
    with pytest.raises(AssertionError, match=r"out \(2051 x torch.bfloat16\), band before: 2 byte\(s\) changed, bytes -2 .. -1"):
        arena.check()
    arena.buf[front : front + 2] = 0xFF
    arena.check()
    out[2050] = float("nan")
    arena.buf[out.data_ptr() - arena.buf.data_ptr() + 2 * 2050 :][:2] = 0xFF
    with pytest.raises(AssertionError, match="1 element\\(s\\) never written, the first at index 2050"):
        arena.assert_written("out")


# ---- skr_noise_random, skr_noise_brownian ------------------------------------------------------------------------------------------
SAMPLE_NUMELS = (5, 37, 105, 8, 2048)


def white32(gpu, seeds, stream: int, n: int) -> torch.Tensor:
    "the fp32 draw into a plain tensor, checked against the oracle's normals"
    out = torch.empty(len(seeds) * n, dtype=torch.float32, device=gpu.dev)
    ok(gpu, gpu.lib.skr_noise_random(out.data_ptr(), _hip.F32, seeds_dev(gpu, seeds).data_ptr(), stream, len(seeds), n, hs(gpu)), "skr_noise_random")
    ref = torch.cat([normal(s, stream, (n,)) for s in seeds])
    assert (out.cpu() - ref).abs().max() < WHITE_BAR
    return out


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off_by_one"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
def test_random(dtype, offset, gpu, arena):
    for batch in (1, 3):
        seeds = SEEDS[:batch]
        for n in SAMPLE_NUMELS:
            arena.reset()
            out = arena.take("out", batch * n, dtype, offset)
            ok(gpu, gpu.lib.skr_noise_random(out.data_ptr(), _hip.DTYPE_CODE[dtype], seeds_dev(gpu, seeds).data_ptr(), 512, batch, n, hs(gpu)), "skr_noise_random")
            settle(arena, "out")
            assert same_draw(out, white32(gpu, seeds, 512, n)), (batch, n)
            if dtype == torch.float32:
                assert (out.cpu() - torch.cat([normal(s, 512, (n,)) for s in seeds])).abs().max() < WHITE_BAR
    product_holds(PN.Random, (2048,), SEEDS, None, [])


def brownian_args(step: Step, hit: bool):
    "what Brownian._batch hands to skr_noise_brownian for this step (the dyadic tree)"
    step = step.normal().clamp()
    t0, t1 = float(step.time_from), float(step.time_to)
    nodes, w_to, w_from = PN.brownian_endpoints(None if hit else t0, t1, PN.brownian_depth(PN.BrownianProps().max_steps), None)
    ids = (ctypes.c_uint64 * len(nodes))(*[PN.BROWNIAN_STREAMS | k for k in nodes])
    wt = (ctypes.c_double * len(nodes))(*w_to)
    wf = None if hit else (ctypes.c_double * len(nodes))(*w_from)
    return ids, wt, wf, len(nodes), 1.0 / math.sqrt(t1 - t0)


@functools.lru_cache(maxsize=None)
def brownian_ref(seed: int, n: int, step: Step) -> torch.Tensor:
    return ON.brownian_noise(seed, (n,), step)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 0), (0, 1)], ids=["aligned", "out_off_by_one", "cache_off_by_one"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
def test_brownian(dtype, offsets, gpu, arena):
    "from_cache 0 then 1: the second query starts where the first ended and reads the banded cache as S_from"
    steps = (Step.from_int(5, 20), Step.from_int(6, 20))
    code = _hip.DTYPE_CODE[dtype]
    for batch in (1, 3):
        seeds = SEEDS[:batch]
        sd = seeds_dev(gpu, seeds)
        for n in SAMPLE_NUMELS:
            arena.reset()
            cache = arena.take("cache", batch * n, torch.float32, offsets[1])
            plain_cache = torch.empty(batch * n, dtype=torch.float32, device=gpu.dev)
            for k, step in enumerate(steps):
                out = arena.take(f"out{k}", batch * n, dtype, offsets[0])
                plain = torch.empty(batch * n, dtype=torch.float32, device=gpu.dev)
                ids, wt, wf, count, scale = brownian_args(step, hit=k == 1)
                ok(gpu, gpu.lib.skr_noise_brownian(out.data_ptr(), code, sd.data_ptr(), ids, wt, wf, count, scale, cache.data_ptr(), k, batch, n, hs(gpu)), "skr_noise_brownian")
                ok(gpu, gpu.lib.skr_noise_brownian(plain.data_ptr(), _hip.F32, sd.data_ptr(), ids, wt, wf, count, scale, plain_cache.data_ptr(), k, batch, n, hs(gpu)), "skr_noise_brownian")
                settle(arena, f"out{k}", "cache")
                ref = torch.cat([brownian_ref(s, n, step) for s in seeds])
                assert rel(plain, ref, "brownian (own specification)", TOL) < TOL, (batch, n, k)
                assert same_draw(out, plain), (batch, n, k)
                assert torch.equal(cache, plain_cache)
            product_holds(PN.Brownian, (n,), seeds, PN.BrownianProps(), [(torch.float32, batch * n)], steps[0])


# ---- skr_noise_offset and its rolling form -------------------------------------------------------------------------------------------
OFFSET_CASES = [((3, 5), PN.OffsetProps(dims=(-1,))), ((4, 33, 20), PN.OffsetProps(dims=(0, 2), strength=0.5)), ((4, 8, 16), PN.OffsetProps(dims=(-1,))),
                ((4, 8, 16), PN.OffsetProps(dims=(0, 2), strength=0.7)), ((2, 3, 4, 2, 2, 8), PN.OffsetProps(dims=(1, 2, 5)))]  # fmt: skip


def offset_ref(unit, props, seed: int, stream: int) -> torch.Tensor:
    dims = tuple(d + len(unit) if d < 0 else d for d in props.dims)
    draws = [normal(seed, stream + 1, ON.offset_shape(unit, dims)), normal(seed, stream, tuple(unit))]
    return ON.offset_noise(unit, ON.Replay(draws).randn, dims, props.strength)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "off_by_one"])
@pytest.mark.parametrize(("unit", "props"), OFFSET_CASES, ids=[f"{u}-{p.dims}" for u, p in OFFSET_CASES])
def test_offset(unit, props, offset, gpu, arena):
    seeds = (11, 12)
    sizes, mask = PN.Offset._merged(unit, props)
    numel = 2 * math.prod(unit)
    draw32 = None
    for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
        arena.reset()
        out = arena.take("out", numel, dtype, offset)
        ok(gpu, gpu.lib.skr_noise_offset(out.data_ptr(), _hip.DTYPE_CODE[dtype], seeds_dev(gpu, seeds).data_ptr(), 256, 257, 2, i64s(sizes), len(sizes), mask, float(props.strength), hs(gpu)), "skr_noise_offset")
        settle(arena, "out")
        if dtype == torch.float32:
            draw32 = out.clone()
            ref = torch.stack([offset_ref(unit, props, s, 256) for s in seeds])
            assert rel(out.reshape(ref.shape), ref, "offset", TOL) < TOL
        assert same_draw(out, draw32), dtype
    product_holds(PN.Offset, unit, seeds, props, [])


@pytest.mark.parametrize("dtype", DTYPES[:3], ids=dtype_ids)
def test_offset_rolling_leaves_inactive_slots_alone(dtype, gpu, arena):
    unit, props, capacity, rows = (4, 8, 16), PN.OffsetProps(), 5, 4
    per = math.prod(unit)
    sizes, mask = PN.Offset._merged(unit, props)
    seeds = [101, 102, 103, 104, 105]
    draws = [2, None, 0, None, 3]
    index = torch.tensor([b * rows + d if d is not None else -1 - b for b, d in enumerate(draws)], dtype=torch.int32, device=gpu.dev)
    out = arena.take("out", capacity * per, dtype)
    code = _hip.DTYPE_CODE[dtype]
    status = gpu.lib.skr_noise_offset_rolling(out.data_ptr(), code, seeds_dev(gpu, seeds).data_ptr(), index.data_ptr(), rows, 256, 0, capacity, i64s(sizes), len(sizes), mask, float(props.strength), hs(gpu))
    ok(gpu, status, "skr_noise_offset_rolling")
    torch.cuda.synchronize()
    arena.check()
    for b, d in enumerate(draws):
        mine = out[b * per : (b + 1) * per]
        if d is None:
            assert untouched(mine), b
            continue
        alone = torch.empty(per, dtype=dtype, device=gpu.dev)
        ok(gpu, gpu.lib.skr_noise_offset(alone.data_ptr(), code, seeds_dev(gpu, [seeds[b]]).data_ptr(), d * 256, d * 256 + 1, 1, i64s(sizes), len(sizes), mask, float(props.strength), hs(gpu)), "skr_noise_offset")
        assert torch.equal(mine, alone) and torch.isfinite(mine.float()).all(), b
        if dtype == torch.float32:
            assert rel(mine.reshape(unit), offset_ref(unit, props, seeds[b], d * 256), "offset", TOL) < TOL


# ---- skr_noise_pyramid: the LDS kernels and their rolling form -----------------------------------------------------------------------
# (lead, h, w, resize_h); the last plane is the largest the level stage takes: 190 * 190 + 47 * 47 + 11 * 11 + 64 of its 38 912 floats
PYRAMID_LDS = [(1, 4, 4, 1), (2, 16, 16, 1), (3, 8, 12, 1), (4, 1, 16, 0), (1, 380, 380, 1)]


def pyramid_unit(lead, h, w, resize_h):
    return ((lead, h, w), {}) if resize_h else ((lead, w), dict(dims=(-1,)))


def pyramid_ref(unit, kw, seed: int, stream: int, with_base: bool) -> torch.Tensor:
    if with_base:
        return pyramid_reference(unit, seed, stream, **kw)
    uniforms = iter(uniform01(np.array([seed], dtype=np.uint64), stream + 255, 8)[0].tolist())
    level = iter(range(8))
    return ON.pyramid_component(unit, lambda shape: spec_normal(seed, stream + 1 + next(level), shape), lambda: next(uniforms), **kw)


@pytest.mark.parametrize("with_base", [1, 0], ids=["with_base", "component"])
@pytest.mark.parametrize("shape", PYRAMID_LDS, ids=str)
def test_pyramid_lds(shape, with_base, gpu, arena):
    lead, h, w, resize_h = shape
    unit, kw = pyramid_unit(*shape)
    seeds, batch, per = (21, 22), 2, lead * h * w
    sd = seeds_dev(gpu, seeds)
    draw32 = None
    for dtype in (torch.float32, torch.bfloat16):
        arena.reset()
        out = arena.take("out", batch * per, dtype)
        scratch = arena.take("scratch_f32", batch * per, torch.float32)
        partials = arena.take("partials_f64", batch * lead * 2, torch.float64)
        level_ws = arena.take("level_ws", batch * 17, torch.int32)
        status = gpu.lib.skr_noise_pyramid(out.data_ptr(), _hip.DTYPE_CODE[dtype], scratch.data_ptr(), partials.data_ptr(), level_ws.data_ptr(), sd.data_ptr(), 256, 256, batch,
                                           lead, h, w, resize_h, 0.3, 99, with_base, hs(gpu))  # fmt: skip
        ok(gpu, status, "skr_noise_pyramid")
        settle(arena, "out")
        if dtype == torch.float32:
            draw32 = out.clone()
            ref = torch.stack([pyramid_ref(unit, kw, s, 256, bool(with_base)) for s in seeds])
            assert rel(out.reshape(ref.shape), ref, "pyramid (LDS kernels)", PYRAMID_TOL) < PYRAMID_TOL
        assert same_draw(out, draw32)
    if with_base:
        product_holds(PN.Pyramid, unit, seeds, PN.PyramidProps(**kw), [(torch.float32, batch * per), (torch.float64, batch * lead * 2), (torch.int32, batch * 17)])


@pytest.mark.parametrize("dtype", DTYPES[:3], ids=dtype_ids)
def test_pyramid_rolling_leaves_inactive_slots_alone(dtype, gpu, arena):
    lead, h, w, capacity, rows = 2, 16, 16, 5, 4
    per = lead * h * w
    seeds = [201, 202, 203, 204, 205]
    draws = [1, None, 3, None, 0]
    index = torch.tensor([b * rows + d if d is not None else -1 - b for b, d in enumerate(draws)], dtype=torch.int32, device=gpu.dev)
    out = arena.take("out", capacity * per, dtype)
    scratch = arena.take("scratch_f32", capacity * per, torch.float32)
    partials = arena.take("partials_f64", capacity * lead * 2, torch.float64)
    level_ws = arena.take("level_ws", capacity * 17, torch.int32)
    code = _hip.DTYPE_CODE[dtype]
    status = gpu.lib.skr_noise_pyramid_rolling(out.data_ptr(), code, scratch.data_ptr(), partials.data_ptr(), level_ws.data_ptr(), seeds_dev(gpu, seeds).data_ptr(), index.data_ptr(), rows,
                                               256, 0, capacity, lead, h, w, 1, 0.3, 99, hs(gpu))  # fmt: skip
    ok(gpu, status, "skr_noise_pyramid_rolling")
    torch.cuda.synchronize()
    arena.check()
    for b, d in enumerate(draws):
        mine = out[b * per : (b + 1) * per]
        if d is None:  # the header's promise: out, scratch_f32, partials_f64 and level_ws keep their bytes there
            assert untouched(mine) and untouched(scratch[b * per : (b + 1) * per]) and untouched(partials[b * lead * 2 : (b + 1) * lead * 2]), b
            assert untouched(level_ws[b * 16 : (b + 1) * 16]) and untouched(level_ws[capacity * 16 + b : capacity * 16 + b + 1]), b
            continue
        alone = torch.empty(per, dtype=dtype, device=gpu.dev)
        ws = PN.Pyramid._lds_workspace(1, per, lead, gpu.dev)
        status = gpu.lib.skr_noise_pyramid(alone.data_ptr(), code, ws[0].data_ptr(), ws[2].data_ptr(), ws[1].data_ptr(), seeds_dev(gpu, [seeds[b]]).data_ptr(), d * 256, d * 256, 1, lead, h, w, 1,
                                           0.3, 99, 1, hs(gpu))  # fmt: skip
        ok(gpu, status, "skr_noise_pyramid")
        assert torch.equal(mine, alone) and torch.isfinite(mine.float()).all(), b
        if dtype == torch.float32:
            assert rel(mine.reshape(lead, h, w), pyramid_reference((lead, h, w), seeds[b], d * 256), "pyramid (LDS kernels)", PYRAMID_TOL) < PYRAMID_TOL


# ---- skr_noise_pyramid_any, skr_noise_pyramid_nd -----------------------------------------------------------------------------------
def python_slots(unit_numel: int) -> int:
    return max(1, min(1024, -(-unit_numel // (4 * 256 * 8))))  # Pyramid._batch


# (unit, PyramidProps arguments); the last resizes axes (0, 1) of three: the second resized axis is not trailing (skr_noise_pyramid_nd)
PYRAMID_ANY = [((2, 7), dict(dims=(-1,))), ((3, 27, 18), {}), ((1, 30, 90), {}), ((6, 10, 12), dict(dims=(0, 1)))]


@pytest.mark.parametrize(("unit", "kw"), PYRAMID_ANY, ids=[str(u) for u, _ in PYRAMID_ANY])
def test_pyramid_any_shape(unit, kw, gpu, arena):
    props = PN.PyramidProps(**kw)
    entry, shape_args, _ = PN.Pyramid._plan(unit, props)
    if entry == "skr_noise_pyramid":  # the any-shape entry under the LDS entry's arguments
        entry = "skr_noise_pyramid_any"
    else:
        assert entry == "skr_noise_pyramid_nd" and unit == (6, 10, 12)
    seeds, batch, per = (41, 42), 2, math.prod(unit)
    sd = seeds_dev(gpu, seeds)
    ref = torch.stack([pyramid_reference(unit, s, 256, **kw) for s in seeds])
    # one slot, the product's count, and more slots than the unit has 2048-element spans: workgroups without work must still leave their slot summable
    for n_slots in sorted({1, python_slots(per), per // 2048 + 7}):
        for dtype in (torch.float32, torch.float16):
            arena.reset()
            out = arena.take("out", batch * per, dtype)
            scratch = arena.take("scratch_f32", batch * per, torch.float32)
            levels = arena.take("levels_f32", batch * per, torch.float32)
            partials = arena.take("partials_f64", batch * n_slots * 2, torch.float64)
            level_ws = arena.take("level_ws", batch * 17, torch.int32)
            status = getattr(gpu.lib, entry)(out.data_ptr(), _hip.DTYPE_CODE[dtype], scratch.data_ptr(), levels.data_ptr(), partials.data_ptr(), n_slots, level_ws.data_ptr(), sd.data_ptr(), 256, 256,
                                             batch, *shape_args, 0.3, 99, 1, hs(gpu))  # fmt: skip
            ok(gpu, status, entry)
            settle(arena, "out")
            if dtype == torch.float32:
                draw32 = out.clone()
                assert rel(out.reshape(ref.shape), ref, "pyramid (any-shape kernels)", PYRAMID_TOL) < PYRAMID_TOL, n_slots
            assert same_draw(out, draw32), n_slots
    n = python_slots(per)
    product_holds(PN.Pyramid, unit, seeds, props, [(torch.float32, batch * per), (torch.float32, batch * per), (torch.float64, batch * n * 2), (torch.int32, batch * 17)])


# ---- skr_noise_colored: one shape per route of choose_route and per branch inside it -------------------------------------------------
def header_slots(d1: int, d2: int, d3: int) -> int:
    "the smallest partial_slots include/skrample_hip.h documents as sufficient for skr_noise_colored"
    return max(d1, -(-(d1 * d2) // max(1, 4096 // d3)))


def python_colored_slots(dims) -> int:
    unit = math.prod(dims)
    return max(256, -(-(unit // dims[-1]) // max(2, 2 * (256 // dims[-1]))))  # Colored._batch


COLORED_ROUTES = {
    "mixed_2d": (56, 88),
    "mixed_3d": (8, 24, 12),  # (the header's formula before this test gave 1 slot here, and the Mixed route declined)
    "fused_planes_2d": (64, 64),
    "fused_planes_3d": (4, 16, 16),
    "fused_planes_inverse128": (4, 128, 128),  # the persistent inverse and its bookkeeping tail
    "passes_direct_out": (8, 128, 256),
    "passes_mid_axes": (2, 256, 256),
    "passes_2d": (256, 256),
}
COLORED_STEP = Step(0.45, 0.5)
# What shows which kernels ran, since a draw names no route:
#   the persistent 128 x 128 inverse counts its launches (skr_stat "colored_inv128_launches"): one per draw of (4, 128, 128), none elsewhere.
#     With batch 1 or 3 every block has one plane, so the ticketed deal of that kernel (more than two planes per block) is not exercised here;
#     tests/test_colored_whole_batch_gpu.py runs it.
#   colored_mid_axes leaves one coloured slot per tile behind the white ones.  (2, 256, 256) has 16 workgroups in its last-axis pass and,
#     at these batches, 33 tiles of four columns, so the kernel runs when 33 <= 2 * partial_slots - 16: from 25 slots on -- at the
#     documented minimum (32) and at the product's count (256), not at the accepted minimum (16), where the separate passes run and the
#     outer-axis kernel writes min(2 * partial_slots - 16, 129) coloured slots.  The doubles of `partials_f64` that were written tell the
#     two apart: 2 * batch * (16 + 33) under colored_mid_axes.  25 slots is run as well: the 49 slots in use end one short of the buffer.
MID_AXES = {"white_slots": 16, "tiles": 33, "first_slots": 25}


@functools.lru_cache(maxsize=None)
def colored_ref(unit: tuple, seed: int, stream: int) -> torch.Tensor:
    return ON.colored_noise(unit, lambda shape: spec_normal(seed, stream, shape), COLORED_STEP)


def smallest_accepted_slots(gpu, dims, batch: int, upto: int) -> int:
    "the smallest partial_slots skr_noise_colored takes for this unit: it refuses before it launches, so only the last probe draws (into plain buffers)"
    d1, d2, d3 = ([1] + list(dims))[-3:]
    unit = math.prod(dims)
    out = torch.empty(batch * unit, dtype=torch.float32, device=gpu.dev)
    spec = torch.empty(batch * (unit // d3) * (d3 // 2 + 1), dtype=torch.complex64, device=gpu.dev)
    scratch = torch.empty(batch * unit, dtype=torch.float32, device=gpu.dev)
    partials = torch.empty(4 * batch * upto, dtype=torch.float64, device=gpu.dev)
    sd = seeds_dev(gpu, SEEDS[:batch])
    for slots in range(1, upto + 1):
        status = gpu.lib.skr_noise_colored(out.data_ptr(), _hip.F32, spec.data_ptr(), scratch.data_ptr(), partials.data_ptr(), slots, sd.data_ptr(), 256, batch, d1, d2, d3, 1.0, 0, 0.0, hs(gpu))
        if status == 0:
            return slots
        assert status in (5, 7), status  # SKR_ERR_SHAPE / SKR_ERR_UNSUPPORTED
    raise AssertionError(f"skr_noise_colored refuses {dims} with up to {upto} slots")


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("route", list(COLORED_ROUTES))
def test_colored_routes(route, batch, gpu, arena):
    dims = COLORED_ROUTES[route]
    d1, d2, d3 = ([1] + list(dims))[-3:]
    unit, seeds = math.prod(dims), SEEDS[:batch]
    half = (unit // d3) * (d3 // 2 + 1)
    documented, python = header_slots(d1, d2, d3), python_colored_slots(dims)
    accepted = smallest_accepted_slots(gpu, dims, batch, documented)  # (the documented minimum is sufficient: the probe ends there at the latest)
    exponent = PN.colored_exponent(COLORED_STEP, PN.ColoredProps())
    sd = seeds_dev(gpu, seeds)
    ref = torch.stack([colored_ref(tuple(dims), s, 256) for s in seeds])
    mid_axes_slots = {MID_AXES["first_slots"]} if route == "passes_mid_axes" else set()
    for slots in sorted({accepted, documented, python} | mid_axes_slots):
        for dtype in (torch.float32, torch.bfloat16):
            inverse128 = gpu.lib.skr_stat(b"colored_inv128_launches")
            arena.reset()
            out = arena.take("out", batch * unit, dtype)
            spec = arena.take("spec_c64", batch * half, torch.complex64)
            scratch = arena.take("scratch_f32", batch * unit, torch.float32)
            partials = arena.take("partials_f64", 4 * batch * slots, torch.float64)
            status = gpu.lib.skr_noise_colored(out.data_ptr(), _hip.DTYPE_CODE[dtype], spec.data_ptr(), scratch.data_ptr(), partials.data_ptr(), slots, sd.data_ptr(), 256, batch, d1, d2, d3,
                                               float(exponent), 0, 0.0, hs(gpu))  # fmt: skip
            ok(gpu, status, f"skr_noise_colored with {slots} slots")
            settle(arena, "out")
            assert gpu.lib.skr_stat(b"colored_inv128_launches") - inverse128 == int(route == "fused_planes_inverse128"), slots
            if route == "passes_mid_axes":
                written = partials.numel() - arena.unwritten("partials_f64").numel()
                fused = 2 * batch * (MID_AXES["white_slots"] + MID_AXES["tiles"])
                assert (written == fused) == (slots >= MID_AXES["first_slots"]), (slots, written)
            if dtype == torch.float32:
                draw32 = out.clone()
                assert rel(out.reshape(ref.shape), ref, "colored", COLORED_TOL) < COLORED_TOL, slots
            assert same_draw(out, draw32), slots
    if batch == 3:
        product_holds(PN.Colored, dims, seeds, PN.ColoredProps(), [(torch.complex64, batch * half), (torch.float32, batch * unit), (torch.float64, 4 * batch * python)], COLORED_STEP)


# ---- skr_noise_colored_any, skr_colorize: partials of exactly 4 * batch * 256 doubles ---------------------------------------------
COLORED_ANY = {
    "direct_2a_3_5": (2, 30, 40),
    "bluestein": (4, 17, 19),
    "four_step_last_axis": (2, 4100),
    "four_axes": (3, 4, 6, 8),
    "seven_axes": (2, 3, 2, 2, 3, 4, 6),
}


@pytest.mark.parametrize("entry", ["skr_noise_colored_any", "skr_colorize"])
@pytest.mark.parametrize("shape", list(COLORED_ANY))
def test_colored_any_shape(shape, entry, gpu, arena):
    dims = COLORED_ANY[shape]
    unit, seeds, batch = math.prod(dims), SEEDS[:2], 2
    half = (unit // dims[-1]) * (dims[-1] // 2 + 1)
    exponent = PN.colored_exponent(COLORED_STEP, PN.ColoredProps())
    sd = seeds_dev(gpu, seeds)
    white = torch.cat([normal(s, 256, tuple(dims)).reshape(-1) for s in seeds]).to(gpu.dev)
    ref = torch.stack([colored_ref(tuple(dims), s, 256) for s in seeds])

    def run(out, spec, work, partials, dtype):
        if entry == "skr_colorize":
            work.copy_(white)  # (the caller's white noise: the transform workspace, overwritten)
            return gpu.lib.skr_colorize(out.data_ptr(), _hip.DTYPE_CODE[dtype], spec.data_ptr(), work.data_ptr(), partials.data_ptr(), batch, len(dims), i32s(dims), float(exponent), 0, 0.0, hs(gpu))
        return gpu.lib.skr_noise_colored_any(out.data_ptr(), _hip.DTYPE_CODE[dtype], spec.data_ptr(), work.data_ptr(), partials.data_ptr(), sd.data_ptr(), 256, batch, len(dims), i32s(dims),
                                             float(exponent), 0, 0.0, hs(gpu))  # fmt: skip

    # once eagerly into plain buffers first: the per-length tables are built on first use
    plain = [torch.empty(batch * unit, dtype=torch.float32, device=gpu.dev), torch.empty(batch * half, dtype=torch.complex64, device=gpu.dev),
             torch.empty(batch * unit, dtype=torch.float32, device=gpu.dev), torch.empty(4 * batch * 256, dtype=torch.float64, device=gpu.dev)]  # fmt: skip
    ok(gpu, run(*plain, torch.float32), entry)
    torch.cuda.synchronize()
    for dtype in (torch.float32, torch.bfloat16):
        arena.reset()
        out = arena.take("out", batch * unit, dtype)
        spec = arena.take("spec_c64", batch * half, torch.complex64)
        work = arena.take("scratch_f32", batch * unit, torch.float32)
        partials = arena.take("partials_f64", 4 * batch * 256, torch.float64)
        ok(gpu, run(out, spec, work, partials, dtype), entry)
        settle(arena, "out")
        if dtype == torch.float32:
            draw32 = out.clone()
            assert rel(out.reshape(ref.shape), ref, "colored", COLORED_TOL) < COLORED_TOL
            assert torch.equal(out, plain[0])
        assert same_draw(out, draw32)
    if entry == "skr_noise_colored_any":
        product_holds(PN.Colored, dims, seeds, PN.ColoredProps(), [(torch.complex64, batch * half), (torch.float32, batch * unit), (torch.float64, 4 * batch * 256)], COLORED_STEP)


# ---- the guidance statistic, skr_error_mean, skr_rolling_advance ---------------------------------------------------------------------
def guidance_inputs(gpu, dtype, numel: int):
    g = torch.Generator().manual_seed(numel)
    uncond = (torch.randn(numel, generator=g) * 0.8 + 0.25).to(dtype).to(gpu.dev)
    cond = (torch.randn(numel, generator=g) * 1.1 - 0.5).to(dtype).to(gpu.dev)
    return uncond, cond


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
def test_guidance_rescale_factor(dtype, batch, gpu, arena):
    code = _hip.DTYPE_CODE[dtype]
    for n in (8, 300, 2048, 2049, 6144):
        arena.reset()
        numel = batch * n
        uncond, cond = guidance_inputs(gpu, dtype, numel)
        count = 4 * batch * ((n + 2047) // 2048)  # SKR_GUIDANCE_PARTIALS(numel, n)
        assert count == _hip.guidance_partials(numel, n)
        factor = arena.take("factor_dev", batch, dtype, offset_elems=1)  # (the header: factor_dev needs the alignment of T only)
        stats = arena.take("stats_dev", 2 * batch, torch.float64)
        partials = arena.take("partials_dev", count, torch.float64)
        plain_factor, plain_stats = torch.empty(batch, dtype=dtype, device=gpu.dev), torch.empty(2 * batch, dtype=torch.float64, device=gpu.dev)
        plain_partials = torch.empty(count, dtype=torch.float64, device=gpu.dev)
        for f, s, p in ((factor, stats, partials), (plain_factor, plain_stats, plain_partials)):
            ok(gpu, gpu.lib.skr_guidance_rescale_factor(uncond.data_ptr(), cond.data_ptr(), code, 7.5, numel, n, f.data_ptr(), s.data_ptr(), p.data_ptr(), hs(gpu)), "skr_guidance_rescale_factor")
        settle(arena, "factor_dev", "stats_dev", "partials_dev")
        assert torch.equal(factor, plain_factor) and torch.equal(stats, plain_stats) and torch.equal(partials, plain_partials), n


@pytest.mark.parametrize("form", ["rolling", "indexed", "indexed_per_sample"])
def test_guidance_rescale_factor_row_forms(form, gpu, arena):
    dtype, batch, n = torch.bfloat16, 3, 2 * 2048
    numel, code, spans = batch * n, _hip.BF16, 2
    uncond, cond = guidance_inputs(gpu, dtype, numel)
    rows = (_hip.StepRowC * 4)()
    for r, row in enumerate(rows):
        row.convert_k[0], row.convert_k[1] = 3.0 + r, 0.7
    rows_dev = TC.rows_tensor(rows).to(gpu.dev)
    picks = {"rolling": [2, -1, 0], "indexed": [1], "indexed_per_sample": [2, 0, 1]}[form]
    index = torch.tensor(picks, dtype=torch.int32, device=gpu.dev)
    factor = arena.take("factor_dev", batch, dtype, offset_elems=1)
    stats = arena.take("stats_dev", 2 * batch, torch.float64)
    partials = arena.take("partials_dev", 4 * batch * spans, torch.float64)
    entry = getattr(gpu.lib, f"skr_guidance_rescale_factor_{form}")
    ok(gpu, entry(uncond.data_ptr(), cond.data_ptr(), code, numel, n, rows_dev.data_ptr(), index.data_ptr(), 1, factor.data_ptr(), stats.data_ptr(), partials.data_ptr(), hs(gpu)), entry.__name__)
    torch.cuda.synchronize()
    arena.check()
    for s in range(batch):
        pick = picks[s] if form != "indexed" else picks[0]
        mine = (factor[s : s + 1], stats[2 * s : 2 * s + 2], partials[4 * spans * s : 4 * spans * (s + 1)])
        if pick < 0:  # inactive: factor_dev[s], its two statistics and its partials keep their bytes
            assert all(untouched(t) for t in mine), s
            continue
        alone = (torch.empty(1, dtype=dtype, device=gpu.dev), torch.empty(2, dtype=torch.float64, device=gpu.dev), torch.empty(4 * spans, dtype=torch.float64, device=gpu.dev))
        status = gpu.lib.skr_guidance_rescale_factor(uncond[s * n :].data_ptr(), cond[s * n :].data_ptr(), code, rows[pick + 1].convert_k[0], n, n, *[t.data_ptr() for t in alone], hs(gpu))
        ok(gpu, status, "skr_guidance_rescale_factor")
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) and torch.isfinite(a.double()).all() for a, b in zip(mine, alone)), s


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
def test_error_mean(dtype, gpu, arena):
    code = _hip.DTYPE_CODE[dtype]
    for numel in (5, 3 * 2048 + 1, 2**20):
        g = torch.Generator().manual_seed(numel)
        a, b = (torch.randn(numel, generator=g).to(dtype).to(gpu.dev) for _ in range(2))
        for power in (1, 2):
            for first in (a, None):
                arena.reset()
                out = arena.take("out_dev", 1, torch.float64)
                partials = arena.take("partials_dev", 1024, torch.float64)
                plain = torch.empty(1025, dtype=torch.float64, device=gpu.dev)
                first_ptr = first.data_ptr() if first is not None else None
                ok(gpu, gpu.lib.skr_error_mean(first_ptr, b.data_ptr(), code, numel, power, out.data_ptr(), partials.data_ptr(), hs(gpu)), "skr_error_mean")
                ok(gpu, gpu.lib.skr_error_mean(first_ptr, b.data_ptr(), code, numel, power, plain.data_ptr(), plain[1:].data_ptr(), hs(gpu)), "skr_error_mean")
                settle(arena, "out_dev")
                assert torch.equal(out, plain[:1]), (numel, power, first is None)


@pytest.mark.parametrize("capacity", [1, 5, 64, 257])
def test_rolling_advance(capacity, gpu, arena):
    max_steps = 3
    position = [(b * 7) % 5 - 1 for b in range(capacity)]  # -1 .. 3: negative, running, finished and beyond
    length = [(b * 3) % 5 for b in range(capacity)]  # 0 (free) .. 4 (longer than max_steps: inactive)
    times = [1000.0 - 0.5 * i for i in range(capacity * max_steps)]
    want_position, want_index, want_time = advance_reference(position, length, times, max_steps)
    position_dev = arena.take("position_dev", capacity, torch.int32)
    index_dev = arena.take("sample_index_dev", capacity, torch.int32)
    timesteps_dev = arena.take("timesteps_dev", capacity, torch.float32)
    position_dev.copy_(torch.tensor(position, dtype=torch.int32))
    length_dev = torch.tensor(length, dtype=torch.int32, device=gpu.dev)
    times_dev = torch.tensor(times, dtype=torch.float32, device=gpu.dev)
    status = gpu.lib.skr_rolling_advance(position_dev.data_ptr(), length_dev.data_ptr(), times_dev.data_ptr(), index_dev.data_ptr(), timesteps_dev.data_ptr(), capacity, max_steps, hs(gpu))
    ok(gpu, status, "skr_rolling_advance")
    torch.cuda.synchronize()
    arena.check()
    assert position_dev.tolist() == want_position and index_dev.tolist() == want_index
    for b, t in enumerate(want_time):
        if t is None:
            assert untouched(timesteps_dev[b : b + 1]), b  # an inactive slot keeps the bytes of its timestep
        else:
            assert timesteps_dev[b].item() == t, b
    assert capacity == 1 or (any(t is None for t in want_time) and any(t is not None for t in want_time))


# ---- the elementwise families: one launch per kernel file, outputs banded, against the same launch into plain tensors ------------------
NUMELS = (5, 37, 2048, 2048 + 3, 8 * 511 + 3, 3 * 2048)
WHOLE = tuple(n for n in NUMELS if n % 2048 == 0)


def contained(gpu, arena, outputs: dict, launch, what: str) -> dict:
    """the generic driver: `launch(pointers)` once into plain tensors and once into arena views of exactly the outputs' sizes
    (`outputs`: name -> (numel, dtype)); the bands stay clean, every output is written and finite and has the plain launch's bits"""
    arena.reset()
    plain = {k: torch.zeros(n, dtype=dt, device=gpu.dev) for k, (n, dt) in outputs.items()}
    banded = {k: arena.take(k, n, dt) for k, (n, dt) in outputs.items()}
    for group in (plain, banded):
        ok(gpu, launch({k: t.data_ptr() for k, t in group.items()}), what)
    settle(arena, *outputs)
    for k in outputs:
        assert torch.equal(banded[k], plain[k]), (what, k)
    return banded


def operands(gpu, dtype, count: int, numel: int) -> list:
    g = torch.Generator().manual_seed(1000 * count + numel)
    return [(torch.randn(numel, generator=g) * (0.5 + 0.25 * k)).to(dtype).to(gpu.dev) for k in range(count)]


def pointers(tensors):
    return (ctypes.c_void_p * max(len(tensors), 1))(*[t if isinstance(t, int) else t.data_ptr() for t in tensors])


def step_plan(n_terms: int, code: int, out0: int, out1: int = _hip.NONE, noise: bool = False, sample: int = 0, n_group_a: int | None = None, dtype_b: int | None = None) -> _hip.StepPlanC:
    p = _hip.StepPlanC()
    p.n_terms, p.n_group_a = n_terms, n_terms if n_group_a is None else n_group_a
    p.dtype_a, p.dtype_b = code, code if dtype_b is None else dtype_b
    p.out0_dtype, p.out1_dtype, p.acc_f64 = out0, out1, int(code == _hip.F64)
    p.noise_mode, p.sample_numel = int(noise), sample
    for k in range(n_terms):
        p.coef0[k], p.coef1[k] = (0.9 - 0.13 * k) * (-1) ** k, 0.2 + 0.07 * k
    if noise:
        p.zeta0, p.stream0 = 0.625, 5
    if out1 != _hip.NONE:
        p.chain = -0.4375
        if noise:
            p.zeta1, p.stream1 = 0.5, 9
    return p


def draws(numel: int) -> bool:
    "a launch that draws needs samples of whole 8-element vectors (skr_step_launch: SKR_ERR_UNSUPPORTED otherwise); the ragged sizes run without noise"
    return numel % 8 == 0


def one_seed(gpu):
    return seeds_dev(gpu, [77])


# (the two-output kernels are instantiated for 16-bit states only; the rounded conversion is evaluated in the tensors' own arithmetic)
# "fp32_out": 16-bit operands under an fp32 output, every size
# "general": sizes that miss the whole-chunk kernels -- 2048 + 8 among them, a ragged size whose one sample still admits a draw, so that the
# general kernel runs WITH its noise path in every dtype -- and, for fp64, which has no one-trip kernel, the whole-chunk sizes as well
STEP_KERNELS = ([(k, t) for k in ("general", "rk_conversion") for t in DTYPES] + [("one_trip", t) for t in DTYPES[:3]]
                + [(k, t) for k in ("two_output", "fp32_out") for t in DTYPES[:2]])  # fmt: skip
RAGGED = tuple(n for n in NUMELS if n % 2048) + (2048 + 8,)


@pytest.mark.parametrize(("kernel", "dtype"), STEP_KERNELS, ids=[f"{k}-{NAMES[t]}" for k, t in STEP_KERNELS])
def test_step_launch(kernel, dtype, gpu, arena):
    code, seeds = _hip.DTYPE_CODE[dtype], one_seed(gpu)
    for numel in {"general": RAGGED + (WHOLE if dtype == torch.float64 else ()), "one_trip": WHOLE}.get(kernel, NUMELS + (2048 + 8,)):
        if kernel == "two_output":  # UniPC-style: four 16-bit operands and the fp32 state, out0 fp32, out1 16-bit
            plan = step_plan(5, code, _hip.F32, code, noise=draws(numel), sample=numel, n_group_a=4, dtype_b=_hip.F32)
            ins = operands(gpu, dtype, 4, numel) + operands(gpu, torch.float32, 1, numel)
            outs = {"out0": (numel, torch.float32), "out1": (numel, dtype)}
        elif kernel == "rk_conversion":
            plan = step_plan(4, code, code, code, noise=draws(numel), sample=numel)
            plan.convert_to, plan.convert_from = 1, 2
            plan.zeta0 = 0.0  # (a Runge-Kutta stage draws on out1 alone)
            for i, k in enumerate((0.83, 0.21, 0.78, 0.41)):
                plan.convert_k[i] = k
            ins = operands(gpu, dtype, 4, numel)
            outs = {"out0": (numel, dtype), "out1": (numel, dtype)}
        else:
            out_dtype = torch.float32 if kernel == "fp32_out" else dtype
            plan = step_plan(3, code, _hip.DTYPE_CODE[out_dtype], noise=draws(numel), sample=numel)
            ins = operands(gpu, dtype, 3, numel)
            outs = {"out0": (numel, out_dtype)}
        arr = pointers(ins)
        contained(gpu, arena, outs, lambda p: gpu.lib.skr_step_launch(ctypes.byref(plan), arr, p["out0"], p.get("out1"), seeds.data_ptr(), numel, hs(gpu)), f"skr_step_launch {kernel} {numel}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
def test_step_launch_masked(dtype, gpu, arena):
    code, seeds = _hip.DTYPE_CODE[dtype], one_seed(gpu)
    for numel in NUMELS:
        plan = step_plan(3, code, code, noise=draws(numel), sample=numel)
        ins = operands(gpu, dtype, 3, numel)
        mask = torch.rand(numel, generator=torch.Generator().manual_seed(numel)).round().to(dtype).to(gpu.dev)
        desc = _hip.StepMaskC(mask.data_ptr(), code, 0, numel, 0)
        arr = pointers(ins)
        contained(gpu, arena, {"out": (numel, dtype)}, lambda p: gpu.lib.skr_step_launch_masked(ctypes.byref(plan), arr, p["out"], ctypes.byref(desc), seeds.data_ptr(), numel, hs(gpu)),
                  f"skr_step_launch_masked {numel}")  # fmt: skip


@pytest.mark.parametrize("rescaled", [False, True], ids=["guided", "guided_rescaled"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
def test_step_launch_guided(dtype, rescaled, gpu, arena):
    code, seeds = _hip.DTYPE_CODE[dtype], one_seed(gpu)
    factor = torch.tensor([0.875], dtype=dtype, device=gpu.dev)
    for numel in NUMELS:
        plan = step_plan(3, code, code, noise=draws(numel), sample=numel)
        ins = operands(gpu, dtype, 4, numel)
        arr, cond = pointers(ins[:3]), ins[3]
        rescale = _hip.StepRescaleC(factor.data_ptr(), 0.7, numel, 0)

        def launch(p):
            guide = _hip.StepGuidanceC(cond.data_ptr(), p["guided_out"], 7.5, 1, 0)
            if rescaled:
                return gpu.lib.skr_step_launch_guided_rescaled(ctypes.byref(plan), arr, p["out"], ctypes.byref(guide), ctypes.byref(rescale), seeds.data_ptr(), numel, hs(gpu))
            return gpu.lib.skr_step_launch_guided(ctypes.byref(plan), arr, p["out"], ctypes.byref(guide), seeds.data_ptr(), numel, hs(gpu))

        contained(gpu, arena, {"out": (numel, dtype), "guided_out": (numel, dtype)}, launch, f"skr_step_launch_guided{'_rescaled' if rescaled else ''} {numel}")


@pytest.mark.parametrize(("dtype", "channels", "plane"), [(torch.bfloat16, 4, 512), (torch.float16, 8, 768), (torch.float32, 3, 680), (torch.bfloat16, 5, 8), (torch.float64, 4, 514)],
                         ids=["one_trip_bf16", "one_trip_fp16", "general_fp32", "general_small", "general_fp64"])  # fmt: skip
def test_step_launch_channels_last(dtype, channels, plane, gpu, arena):
    code, seeds, numel = _hip.DTYPE_CODE[dtype], one_seed(gpu), channels * plane
    plan = step_plan(3, code, code, noise=draws(numel), sample=numel)
    ins = operands(gpu, dtype, 3, numel)  # (kept: the pointer array does not hold them)
    arr = pointers(ins)
    layout = _hip.StepLayoutC(channels, plane)
    before = {k: gpu.lib.skr_stat(k) for k in (b"channels_last_one_trip", b"channels_last_general")}
    contained(gpu, arena, {"out0": (numel, dtype)}, lambda p: gpu.lib.skr_step_launch_channels_last(ctypes.byref(plan), arr, p["out0"], None, seeds.data_ptr(), ctypes.byref(layout), numel, hs(gpu)),
              "skr_step_launch_channels_last")  # fmt: skip
    took = b"channels_last_one_trip" if numel % 2048 == 0 and dtype in (torch.bfloat16, torch.float16) else b"channels_last_general"
    assert gpu.lib.skr_stat(took) == before[took] + 2


@pytest.mark.parametrize("form", TC.FORMS)
def test_step_launch_row_forms(form, gpu, arena):
    "one each of skr_step_launch_indexed, _indexed_per_sample and _rolling, on the plan and row builders of tests/table_cases.py"
    case, dtype, batch, sample = TC.Case("k1", 3, noise="on"), torch.bfloat16, 4, 2048
    numel = batch * sample
    plan = TC.make_plan(case, _hip.BF16, sample)
    rows, present = TC.build_rows(case, rolling=form == "rolling")
    rows_dev = TC.rows_tensor(rows).to(gpu.dev)
    picks = {"whole": [2], "per_sample": [0, 3, 5, 1], "rolling": [4, -1, len(rows) - 1, -2]}[form]
    index = torch.tensor(picks, dtype=torch.int32, device=gpu.dev)
    seeds = seeds_dev(gpu, TC.seeds_for(batch))
    ins = operands(gpu, dtype, 3, numel)  # (kept: the pointer array does not hold them)
    arr = pointers(ins)
    entry = {"whole": gpu.lib.skr_step_launch_indexed, "per_sample": gpu.lib.skr_step_launch_indexed_per_sample, "rolling": gpu.lib.skr_step_launch_rolling}[form]
    plain = torch.zeros(numel, dtype=dtype, device=gpu.dev)
    out = arena.take("out0", numel, dtype)
    for target in (plain, out):
        ok(gpu, entry(ctypes.byref(plan), arr, target.data_ptr(), None, seeds.data_ptr(), numel, rows_dev.data_ptr(), index.data_ptr(), 0, hs(gpu)), form)
    torch.cuda.synchronize()
    arena.check()
    for s in range(batch):
        mine = out[s * sample : (s + 1) * sample]
        if form == "rolling" and picks[s] < 0:
            assert untouched(mine), s  # an inactive sample: out0 keeps its bytes there
        else:
            assert torch.equal(mine, plain[s * sample : (s + 1) * sample]) and torch.isfinite(mine.float()).all(), s


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
@pytest.mark.parametrize(("masked", "n_grads"), [(False, 3), (False, 17), (True, 3), (True, 16)], ids=["step_3", "step_17", "masked_3", "masked_16"])
def test_step_backward(masked, n_grads, dtype, gpu, arena):
    "skr_step_backward_launch with 3 and 17 gradients; skr_step_masked_backward_launch with 3 and 16 (SKR_ROW_TERMS: it takes no more)"
    code = _hip.DTYPE_CODE[dtype]
    for numel in NUMELS:
        plan = _hip.StepGradPlanC()
        plan.n_grads, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.g0_dtype = n_grads, n_grads, code, code, code
        plan.g1_dtype, plan.acc_f64 = (_hip.NONE if masked else code), int(dtype == torch.float64)
        for k in range(n_grads):
            plan.a[k], plan.b[k] = 0.9 - 0.11 * k, -0.3 + 0.05 * k
        g0, g1, mask = operands(gpu, dtype, 3, numel)
        mask = (mask > 0).to(dtype)
        desc = _hip.StepMaskC(mask.data_ptr(), code, 0, numel, 0)
        names = [f"grad{k}" for k in range(n_grads)]

        def launch(p):
            grads = pointers([p[k] for k in names])
            if masked:
                return gpu.lib.skr_step_masked_backward_launch(ctypes.byref(plan), g0.data_ptr(), ctypes.byref(desc), grads, numel, numel, hs(gpu))
            return gpu.lib.skr_step_backward_launch(ctypes.byref(plan), g0.data_ptr(), g1.data_ptr(), grads, numel, hs(gpu))

        contained(gpu, arena, {k: (numel, dtype) for k in names}, launch, f"backward {numel}")


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_ids)
@pytest.mark.parametrize("tape_words", [1, 2])
def test_tape_launch(tape_words, dtype, gpu, arena):
    tape = _hip.TapeC()
    ops = [(_hip.TAPE_LOAD, 0, 0, 0, 0.0), (_hip.TAPE_LOAD, 1, 1, 0, 0.0), (_hip.TAPE_MUL_S, 0, 0, 0, 0.5), (_hip.TAPE_ADD, 2, 0, 1, 0.0), (_hip.TAPE_SUB_MS, 1, 2, 0, 0.25),
           (_hip.TAPE_STORE, 0, 2, 0, 0.0), (_hip.TAPE_STORE, 0, 1, 1, 0.0)]  # fmt: skip
    tape.n_ops, tape.n_inputs, tape.n_outputs, tape.dtype = len(ops), 2, 2, _hip.DTYPE_CODE[dtype]
    for i, (c, dst, a, b, k) in enumerate(ops):
        tape.ops[i] = _hip.TapeOpC(c, dst, a, b, k)
    assert gpu.lib.skr_set_tuning(b"tape_words", tape_words) == 0
    try:
        for numel in NUMELS:
            ins = operands(gpu, dtype, 2, numel)  # (kept: the pointer array does not hold them)
            arr = pointers(ins)
            contained(gpu, arena, {"out0": (numel, dtype), "out1": (numel, dtype)}, lambda p: gpu.lib.skr_tape_launch(ctypes.byref(tape), arr, pointers([p["out0"], p["out1"]]), numel, hs(gpu)),
                      f"skr_tape_launch {numel}")  # fmt: skip
    finally:
        assert gpu.lib.skr_set_tuning(b"tape_words", 0) == 0


@pytest.mark.parametrize(("out_dtype", "a_dtype", "b_dtype"), [(torch.float32, torch.bfloat16, torch.float32), (torch.float32, torch.float16, torch.float16), (torch.float64, torch.float64, torch.bfloat16)],
                         ids=["fp32_from_bf16_fp32", "fp32_from_fp16", "fp64_from_fp64_bf16"])  # fmt: skip
def test_power_blend_and_backward(out_dtype, a_dtype, b_dtype, gpu, arena):
    oc, ac, bc = (_hip.DTYPE_CODE[t] for t in (out_dtype, a_dtype, b_dtype))
    for numel in NUMELS:
        a, b, g = operands(gpu, a_dtype, 1, numel)[0], operands(gpu, b_dtype, 2, numel)[1], operands(gpu, out_dtype, 3, numel)[2]
        contained(gpu, arena, {"out": (numel, out_dtype)}, lambda p: gpu.lib.skr_power_blend(p["out"], oc, a.data_ptr(), ac, b.data_ptr(), bc, 0.6, 0.4, 2.0, numel, hs(gpu)), f"skr_power_blend {numel}")
        contained(gpu, arena, {"grad_a": (numel, a_dtype), "grad_b": (numel, b_dtype)},
                  lambda p: gpu.lib.skr_power_blend_backward(p["grad_a"], p["grad_b"], g.data_ptr(), oc, a.data_ptr(), ac, b.data_ptr(), bc, 0.6, 0.4, 2.0, numel, hs(gpu)), f"skr_power_blend_backward {numel}")  # fmt: skip
