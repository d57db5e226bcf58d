"""Every noise generator, route and store path in every output dtype against its own fp32 draw, bit for bit over all elements.

The contract (csrc/skr_pack.h): with the same seeds, stream numbers, step and props,
  bf16 / fp16   draw(dtype) has exactly the bits of RNE_dtype(draw(float32)): fp32 arithmetic, then ONE rounding to nearest even;
  float64       draw(float64) is the fp32 draw widened (exact), wherever the kernel's last operation is in fp32.
The reference is the fp32 DEVICE draw copied to the host and rounded by bit_model.round_to (torch's CPU conversion of an fp32 tensor, held
against an integer RNE in tests/test_bit_model_host.py; never through float64, where torch rounds twice); the comparison is on the
integer views (bit_model.same_bits), zero differing elements accepted, no element left out.  The fp32 draws themselves stand on the
oracle tests of tests/test_noise_gpu.py; `test_fp32_random_draws_stand_on_the_oracle` anchors them once more at the sizes used here.

Why 2^21 elements per id.  A store that fuses the last multiply with the conversion (v_fma_mixlo_f16: the exact product rounded once)
differs from the contract only where the fp32 product lands exactly on an fp16 tie and the exact product does not: about 2^-14 of the
elements (tests/noise_dtype_model.py counts 114 to 137 of 2^21 for the last operations below).  2^21 elements expect over 100 differing
ones, so such a store slips through with probability below e^-100; the 1 536 elements of test_vector_and_generic_kernels_agree_bitwise
expect 0.1.  bf16 has no fused conversion on gfx950 (v_cvt_pk_bf16_f32 everywhere) and is held all the same.

Which elements a scalar store reaches.  The compiler turns a grid-stride loop `for (i = thread; i < n; i += stride) out[i] = (T)(x[i] * f)`
(normalise_pass2's scalar branch, any_finish) into a two-wide body and a one-element remainder, and only the remainder held the fused
instruction: the last trip of every thread whose number of trips is odd.  A unit of 2^21 elements under 16 384 threads (128 trips each)
sends two thousand elements there and expects 0.1 differing ones; a unit no longer than the grid sends every element.  Units of both
kinds are drawn -- long ones for the body, and batches of short ones (one or three trips per thread: 255, 252, 768, 120 elements) sized
so that 2^21 elements take the last odd trip -- because what the compiler makes of the body and of the remainder are two store paths.
The one-block-per-Philox-block kernels (random_kernel, brownian_kernel<!ALIGNED>, offset_kernel) have no such split.

  generator   store paths (kernel: what sends a draw there)
  Random      random_kernel_v8 (sample_numel % 8 == 0, 16-byte aligned base) | random_kernel: ragged sample_numel; the base off by one
              element; batch > 65535
  Offset      offset_kernel_v8 | offset_kernel (innermost axis no multiple of 8); an offset per channel, and one per innermost index
  Pyramid     normalise_pass2, vector branch (unit % 4 == 0 and a 16-byte aligned sample) behind the LDS kernels | its scalar branch behind
              the any-shape kernels (unit % 4 != 0), behind skr_noise_pyramid_nd, and -- the parity case -- BOTH branches in one launch:
              a 16-bit unit of 4 * odd elements puts every second sample 8 bytes off a 16-byte boundary
  Colored     colored_last_axis_out, colored_plane, colored_inverse128, colored_plane_mixed, colored_finish (csrc/skr_colored.hip) and
              any_finish (csrc/skr_colored_any.hip: behind colored_planes, behind the own transforms, and for colorize_noise on a caller's
              tensor); units from ARMS of tests/test_colored_routes_gpu.py, batches sized to 2^21 elements; no draw may reach hipFFT
  Brownian    brownian_kernel<ALIGNED> | <!ALIGNED> (odd sample_numel), each on a cache miss and then on a cache hit; fp16 included

float64.  Every store of the generators converts an fp32 value: Random and Offset store the normals / the fp32 sum, normalise_pass2
`src[i] * inv`, Brownian `scale * (to - from)`, any_finish and colored_finish `real * factor`, the plane kernels `z * gain` -- all fp32
products widened by the store; no store computed in double was found.  So float64 is held to the widened fp32 draw exactly, with three
exceptions that are other KERNELS, not other stores: the double instantiations of the plane kernels exist in the run-time-geometry form only
(plane_kernel / mixed_kernel of skr_colored.hip), and colored_inverse128 has no double instantiation (inverse128_blocks), so the
float64 draws of 128 x 128 planes (2-D: colored_plane<2, double, 0, 0> for colored_plane<2, float, 7, 7>; under a leading axis:
colored_plane<1, double, 0, 0> for colored_inverse128<float>) and of 96 x 96 planes (colored_plane_mixed<2, double, 512> for
<2, float, 512, 96>) take the same algorithm through differently contracted multiply-adds
(test_compile_time_geometry_planes_agree_with_the_runtime_kernel) or another factorisation.  Those three ids keep the bar
tests/test_colored_routes_gpu.py holds float64 to: relative inf-norm error below 1e-5 against the fp32 draw."""

import ctypes
import functools

import bit_model as BM
import numpy as np
import pytest
import torch
from skr_oracle import noise as ON

from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.pytorch import noise as PN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CODE = _hip.DTYPE_CODE
DTYPES = [torch.bfloat16, torch.float16, torch.float64]
FLOOR = 1 << 21  # elements per id, at least
TOL = 1e-5  # tests/test_noise_gpu.py::TOL, the bar of every fp32 generator comparison of the suite


def name(dtype) -> str:
    return str(dtype).replace("torch.", "")


def differing(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    "print how many elements of `got` have other bits than `want`, then require none"
    bad = int(BM.differing(got, want).sum())
    print(f"{what} [{name(got.dtype)}]: {bad} of {got.numel()} elements differ in bits")
    BM.same_bits(got, want, what=f"{what} [{name(got.dtype)}]")


def hold(got: torch.Tensor, ref32: torch.Tensor, what: str, report_only: bool = False) -> None:
    """the contract: `got` (a device draw) has the bits of the fp32 draw `ref32` (on the host) rounded once / widened.
    report_only: print the count and leave the requirement to a second call (a test with two draws reports both before it fails on one)"""
    assert ref32.dtype == torch.float32 and not ref32.is_cuda and got.numel() == ref32.numel() >= FLOOR, (what, got.shape, ref32.shape)
    want = ref32.reshape(-1).double() if got.dtype == torch.float64 else BM.round_to(got.dtype, ref32.numpy().reshape(-1))
    if report_only:
        print(f"{what} [{name(got.dtype)}]: {int(BM.differing(got.cpu().reshape(-1), want).sum())} of {got.numel()} elements differ in bits")
    else:
        differing(got.cpu().reshape(-1), want, what)


def seed_vector(batch: int, first: int = 1000) -> torch.Tensor:
    return torch.arange(first, first + batch, dtype=torch.int64, device=DEV)


def hstream() -> int:
    return _hip.current_stream_ptr(DEV)


def into_guarded_buffer(launch, dtype, numel: int, shift: int) -> torch.Tensor:
    "launch(pointer) writes `numel` elements `shift` elements behind a 16-byte aligned base; the elements around them keep their zeros"
    buf = torch.zeros(numel + 8, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[shift : shift + numel]
    launch(out.data_ptr())
    torch.cuda.synchronize()
    assert (buf[:shift] == 0).all() and (buf[shift + numel :] == 0).all(), "a store outside the draw"
    return out


# ---- Random (skr_noise_random, called as tests/test_noise_gpu.py::test_vector_and_generic_kernels_agree_bitwise calls it) ---------------
RANDOM_STREAM = 7 * 256
RANDOM = {  # path: (batch, sample_numel, elements the base is off a 16-byte boundary)
    "v8": (4, 1 << 19, 0),
    "ragged": (3, 699051, 0),
    "shifted": (4, 1 << 19, 1),
    "batch>65535": (65536, 32, 0),
}


def random_draw(path: str, dtype) -> torch.Tensor:
    batch, numel, shift = RANDOM[path]
    seeds, lib = seed_vector(batch), _hip.load()
    return into_guarded_buffer(lambda p: _hip.check(lib.skr_noise_random(p, CODE[dtype], seeds.data_ptr(), RANDOM_STREAM, batch, numel, hstream()), "skr_noise_random"),
                               dtype, batch * numel, shift)  # fmt: skip


@functools.lru_cache(maxsize=None)
def random_ref(path: str) -> torch.Tensor:
    return random_draw(path, torch.float32).cpu()


def test_random_paths_are_the_ones_named():
    "the launcher's rule (launch_random of csrc/skr_api.hip), restated on the cases: only `v8` may take random_kernel_v8"
    for path, (batch, numel, shift) in RANDOM.items():
        fast = numel % 8 == 0 and batch <= 65535 and shift == 0
        assert fast == (path == "v8") and batch * numel >= FLOOR, path


@pytest.mark.parametrize("path", ["v8", "ragged"])
def test_fp32_random_draws_stand_on_the_oracle(path):
    "the anchor of the reference at the sizes used here; and in fp32, too, the base off by one element changes no bit"
    batch, numel, _ = RANDOM[path]
    got = random_ref(path).reshape(batch, numel).double()
    want = torch.from_numpy(np.stack([ON.philox_normal(1000 + b, RANDOM_STREAM, numel) for b in range(batch)])).double()
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f"fp32 Random {path} against oracle.philox_normal: relative inf-norm error {err:.3g} (bar {TOL})")
    assert err < TOL, (path, err)
    if path == "v8":
        differing(random_ref("shifted"), random_ref("v8"), "Random, base off by one element against the aligned base")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("path", list(RANDOM))
def test_random(path, dtype):
    got = random_draw(path, dtype)
    if path == "shifted":  # the generic kernel behind an unaligned base writes the aligned kernel's bits
        hold(got, random_ref(path), f"Random {path}", report_only=True)
        differing(got.cpu(), random_draw("v8", dtype).cpu(), "Random, base off by one element against the aligned base")
    hold(got, random_ref(path), f"Random {path}")


# ---- Offset (skr_noise_offset) ----------------------------------------------------------------------------------------------------------
OFFSET = {  # path: (unit, keep mask: bit k = axis k keeps its size in the offset tensor, batch)
    "v8, an offset per channel": ((4, 256, 512), 0b001, 4),
    "v8, innermost axis kept": ((4, 256, 512), 0b101, 4),
    "generic, an offset per channel": ((5, 333, 315), 0b001, 4),
    "generic, innermost axis kept": ((5, 333, 315), 0b101, 4),
}


def offset_draw(path: str, dtype) -> torch.Tensor:
    unit, mask, batch = OFFSET[path]
    assert (unit[-1] % 8 == 0) == path.startswith("v8")  # (offset_v8_covers of csrc/skr_noise.hip)
    seeds, lib, shape = seed_vector(batch, 2000), _hip.load(), (ctypes.c_int64 * 3)(*unit)
    numel = batch * unit[0] * unit[1] * unit[2]
    return into_guarded_buffer(lambda p: _hip.check(lib.skr_noise_offset(p, CODE[dtype], seeds.data_ptr(), 512, 513, batch, shape, 3, mask, 0.6, hstream()), "skr_noise_offset"),
                               dtype, numel, 0)  # fmt: skip


@functools.lru_cache(maxsize=None)
def offset_ref(path: str) -> torch.Tensor:
    return offset_draw(path, torch.float32).cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("path", list(OFFSET))
def test_offset(path, dtype):
    hold(offset_draw(path, dtype), offset_ref(path), f"Offset {path}")


# ---- Pyramid ----------------------------------------------------------------------------------------------------------------------------
PYRAMID = {  # path: (unit, props, batch, entry point that draws it)
    "LDS kernels, vector normalise": ((4, 256, 256), PN.PyramidProps(), 8, "skr_noise_pyramid"),
    "any-shape kernels, unit % 4 != 0": ((3, 333, 525), PN.PyramidProps(), 4, "skr_noise_pyramid_any"),
    "any-shape kernels, unit % 4 != 0, one trip per thread": ((3, 5, 17), PN.PyramidProps(), 8225, "skr_noise_pyramid_any"),
    "skr_noise_pyramid_nd": ((257, 3, 682), PN.PyramidProps(dims=(0, 2)), 4, "skr_noise_pyramid_nd"),
}
PARITY = {  # units of 4 * odd elements: (unit, seeds)
    "one large unit": ((1, 1023, 2052), [71, 72]),  # 2 099 196 = 4 * 524 799 elements
    "many small units": ((1, 4, 63), list(range(7000, 7000 + 16646))),  # 252 = 4 * 63 elements, one trip per thread; 2^21 elements at odd positions
}


def pyramid_draw(unit, props, seeds, dtype, entry=None) -> torch.Tensor:
    g = PN.BatchTensorNoise.from_batch_inputs(PN.Pyramid, unit, seeds, props=props, dtype=dtype)
    out = g.generate(None)
    torch.cuda.synchronize()
    if entry is not None:  # (the route `_batch` took: the any-shape buffers exist only behind a refusal of the LDS kernels)
        planned = PN.Pyramid._plan(unit, props)[0]
        assert ("skr_noise_pyramid_any" if "any_shape" in g._state else planned) == entry, (unit, planned, sorted(map(str, g._state)))
    return out


@functools.lru_cache(maxsize=None)
def pyramid_ref(path: str) -> torch.Tensor:
    if path in PARITY:
        return pyramid_draw(PARITY[path][0], PN.PyramidProps(), PARITY[path][1], torch.float32, "skr_noise_pyramid_any").cpu()
    unit, props, batch, entry = PYRAMID[path]
    return pyramid_draw(unit, props, list(range(3000, 3000 + batch)), torch.float32, entry).cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("path", list(PYRAMID))
def test_pyramid(path, dtype):
    unit, props, batch, entry = PYRAMID[path]
    numel = unit[0] * unit[1] * unit[2]
    assert (numel % 4 == 0) == (path == "LDS kernels, vector normalise")
    hold(pyramid_draw(unit, props, list(range(3000, 3000 + batch)), dtype, entry), pyramid_ref(path), f"Pyramid {path}")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("path", list(PARITY))
def test_pyramid_sample_bits_do_not_depend_on_the_batch_position(path, dtype):
    """normalise_pass2 picks its branch per sample: `(unit & 3) == 0 && dst 16-byte aligned`.  A 16-bit unit of 4 * odd elements is 8 * odd
    bytes long, so the samples at even positions take the vector branch and those at odd positions the scalar one in the same launch.
    Both must round as the contract says, and a sample must have the bits its seed gets one position further to the front, on the other
    branch: the seeds without the first are drawn again -- for two seeds that is sample 1 drawn alone at position 0.  (float64: samples are
    32 * odd bytes long, every sample takes the vector branch; the id holds the widened draw and the independence of the position.)"""
    (unit, seeds), props = PARITY[path], PN.PyramidProps()
    numel = unit[0] * unit[1] * unit[2]
    assert numel % 4 == 0 and (numel // 4) % 2 == 1 and len(seeds) // 2 * numel >= FLOOR // 2
    whole = pyramid_draw(unit, props, seeds, dtype, "skr_noise_pyramid_any")
    assert whole.data_ptr() % 16 == 0 and whole[1].data_ptr() - whole.data_ptr() == numel * whole.element_size()
    if dtype != torch.float64:
        assert whole[1].data_ptr() % 8 == 0 and whole[1].data_ptr() % 16 != 0, "sample 1 must take the scalar branch"
    moved = pyramid_draw(unit, props, seeds[1:], dtype, "skr_noise_pyramid_any")
    assert moved.data_ptr() % 16 == 0
    hold(whole, pyramid_ref(path), f"Pyramid parity, {path}, even positions (vector branch) and odd ones (scalar branch)", report_only=True)
    differing(moved.cpu().reshape(-1), whole[1:].cpu().reshape(-1), f"Pyramid parity, {path}, every sample one position further to the front")
    hold(whole, pyramid_ref(path), f"Pyramid parity, {path}, even positions (vector branch) and odd ones (scalar branch)")


# ---- Colored ----------------------------------------------------------------------------------------------------------------------------
COLORED = {  # the kernel that stores to `out`: (unit, batch)
    "colored_last_axis_out": ((4, 128, 256), 16),
    "colored_plane": ((128, 128), 128),
    "colored_inverse128": ((2, 128, 128), 64),
    "colored_plane_mixed": ((96, 96), 228),
    "colored_finish": ((128, 256), 64),
    "any_finish behind colored_planes, three trips per thread": ((2, 3, 8, 16), 8192),
    "any_finish behind the own transforms, one trip per thread": ((3, 40), 17477),
    "any_finish behind the own transforms, seven trips per thread": ((4, 720, 1280), 1),
}
OTHER_KERNEL_IN_FLOAT64 = {"colored_plane", "colored_inverse128", "colored_plane_mixed"}  # (the module docstring says why)


def colored_draw(path: str, dtype) -> torch.Tensor:
    "one draw; no colored draw may reach hipFFT, and colored_inverse128 runs for its unit in the dtypes it is compiled for and for nothing else"
    unit, batch = COLORED[path]
    lib = _hip.load()
    before = lib.skr_stat(b"hipfft_execs"), lib.skr_stat(b"colored_inv128_launches")
    out = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, unit, list(range(4000, 4000 + batch)), props=PN.ColoredProps(), dtype=dtype).generate(None)
    torch.cuda.synchronize()
    after = lib.skr_stat(b"hipfft_execs"), lib.skr_stat(b"colored_inv128_launches")
    assert after[0] == before[0], "a colored draw went to hipFFT"
    assert (after[1] > before[1]) == (path == "colored_inverse128" and dtype != torch.float64), (path, dtype, before, after)
    return out


@functools.lru_cache(maxsize=None)
def colored_ref(path: str) -> torch.Tensor:
    return colored_draw(path, torch.float32).cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("path", list(COLORED))
def test_colored(path, dtype):
    got, ref = colored_draw(path, dtype), colored_ref(path)
    if dtype == torch.float64 and path in OTHER_KERNEL_IN_FLOAT64:
        assert got.numel() == ref.numel() >= FLOOR
        want = ref.double()
        err = ((got.cpu() - want).abs().max() / want.abs().max()).item()
        print(f"Colored {path} [float64]: another kernel than the fp32 draw's, relative inf-norm error {err:.3g} (bar {TOL})")
        assert err < TOL, (path, err)
    else:
        hold(got, ref, f"Colored {path}")


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_colorize_noise_on_a_callers_tensor(dtype):
    """colorize_noise widens the caller's tensor to fp32, colours it on the own transforms and stores in the caller's dtype (any_finish): the
    result has the bits of the fp32 result for the same, widened, white noise."""
    lib = _hip.load()
    white32 = torch.randn((3, 700, 1248), generator=torch.Generator().manual_seed(5), dtype=torch.float32)  # (five trips per thread of any_finish)
    white = white32.to(dtype).to(DEV)  # (float64: exact; 16-bit: the rounded values ARE the white noise of both runs)
    before = lib.skr_stat(b"hipfft_execs")
    got = PN.Colored.colorize_noise(white, 0.25)
    ref = PN.Colored.colorize_noise(white.float(), 0.25)
    torch.cuda.synchronize()
    assert lib.skr_stat(b"hipfft_execs") == before, "colorize_noise went to hipFFT"
    assert got.dtype == dtype and ref.dtype == torch.float32 and got.shape == white.shape
    hold(got, ref.cpu(), "colorize_noise (3, 700, 1248)")


# ---- Brownian ---------------------------------------------------------------------------------------------------------------------------
BROWNIAN = {"aligned": ((4, 128, 128), 32), "odd sample_numel": ((3, 333, 525), 4)}  # path: (unit, batch)
BROWNIAN_STEPS = (Step.from_int(5, 20), Step.from_int(6, 20))  # the second starts where the first ended: a cache miss, then a hit


def brownian_draws(path: str, dtype) -> list[torch.Tensor]:
    unit, batch = BROWNIAN[path]
    assert (unit[0] * unit[1] * unit[2] % 8 == 0) == (path == "aligned")  # (launch_brownian of csrc/skr_api.hip)
    g = PN.BatchTensorNoise.from_batch_inputs(PN.Brownian, unit, list(range(5000, 5000 + batch)), props=PN.BrownianProps(), dtype=dtype)
    assert g._state.get("brownian_cache_time") is None
    miss = g.generate(BROWNIAN_STEPS[0])
    assert g._state["brownian_cache_time"] == BROWNIAN_STEPS[1].time_from, "the second step must find W(time_from) cached"
    hit = g.generate(BROWNIAN_STEPS[1])
    torch.cuda.synchronize()
    return [miss, hit]


@functools.lru_cache(maxsize=None)
def brownian_ref(path: str) -> tuple:
    return tuple(d.cpu() for d in brownian_draws(path, torch.float32))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("path", list(BROWNIAN))
def test_brownian(path, dtype):
    draws = list(zip(("cache miss", "cache hit"), brownian_draws(path, dtype), brownian_ref(path)))
    hold(draws[1][1], draws[1][2], f"Brownian {path}, {draws[1][0]}", report_only=True)
    for which, got, ref in draws:
        hold(got, ref, f"Brownian {path}, {which}")
