"""Colored noise on (d1, 128, 128) units, every sample of production-size draws against a float64 evaluation.

The plane pipeline of these units runs three kernels that hand state from workgroup to workgroup: colored_plane<0> resets the
bookkeeping words, colored_outer_axis_regs counts arrivals per sample (the last block of a sample computes its rescale factor), and the
persistent colored_inverse128 (grid G = 2 x CUs) deals every plane past each block's first two from a device ticket -- which it only does
once a draw holds more than 2G planes.  The suite's other Colored tests draw at most a few dozen planes, and the full-size tests compare
three samples, so this module draws on both sides of each grid threshold and holds EVERY sample to a float64 colorize of the white
noise the kernel drew itself:

* the white noise comes from PN.Random with the same seeds: draw n of Random and draw n of Colored both use Philox stream n * 256 and
  normal4 (csrc/skr_philox.h), so Random hands over the very normals the Colored kernel transformed.  That shared stream is what the
  test relies on; were it not so, every comparison below would miss the 1e-5 bar by orders of magnitude, not by a little;
* the float64 colorize restates ON.colorize for a batch (and is pinned to it on two samples at 1e-12);
* fp32 output: max |got - ref| / max |ref| <= 1e-5 per sample (COLORED_TOL of tests/test_noise_gpu.py); 16-bit output: every element
  within one unit in the last place of the reference plus 1e-5 * max |ref| of its sample;
* skr_stat's colored_inv128 counters say which path ran: the persistent kernel on every draw, ticketed exactly when planes > 2G;
* a draw into NaN-filled buffers the test owns shows that no output element is left unwritten (torch.empty could hide one: an unwritten
  plane keeps what the allocator left there, and would even be deterministic);
* the host-selected variants (SKR_COLORED_INV_STATIC / _INV_BLOCKS / _FACTORS_KERNEL / _OLD_INVERSE, read once per process) run in
  fresh child processes.
"""

import json
import math
import os
import subprocess
import sys

import pytest
import torch
from conftest import ROOT, note_margin

from skr_oracle import noise as ON
from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.pytorch import noise as PN

pytestmark = pytest.mark.gpu
COLORED_TOL = 1e-5  # tests/test_noise_gpu.py: fp32 generator outputs, relative inf-norm per sample
ADDITIVE_16 = 1e-5  # 16-bit outputs: beyond one last-place unit of the reference, this much of the sample's max |ref|
H = W = 128
CHUNK = 32  # samples per float64 transform (a 16 x 128 x 128 sample is 2 MB real, 2.1 MB of spectrum)

# name: (planes as a function of the persistent grid G and d1, d1, output dtype).  Every dtype and every d1 meets the ticket (> 2G)
# at least once: fp16 with d1 = 2, bf16 with d1 = 8, fp32 with d1 = 16 and 4, and all three at the cfg3c size.
CASES = {
    "below_G": (lambda G, d1: G // 2, 2, torch.bfloat16),
    "exactly_G": (lambda G, d1: G, 4, torch.float16),
    "between_G_and_2G": (lambda G, d1: 3 * G // 2, 8, torch.float32),
    "exactly_2G": (lambda G, d1: 2 * G, 16, torch.bfloat16),
    "2G_plus_d1_d1=2": (lambda G, d1: 2 * G + d1, 2, torch.float16),
    "2G_plus_d1_d1=8": (lambda G, d1: 2 * G + d1, 8, torch.bfloat16),
    "2G_plus_d1_d1=16": (lambda G, d1: 2 * G + d1, 16, torch.float32),
    "3G_plus_2d1": (lambda G, d1: 3 * G + 2 * d1, 4, torch.float32),
    "cfg3c_bf16": (lambda G, d1: 256 * 16, 16, torch.bfloat16),
    "cfg3c_fp16": (lambda G, d1: 256 * 16, 16, torch.float16),
    "cfg3c_fp32": (lambda G, d1: 256 * 16, 16, torch.float32),
}
STEPS = (None, Step(0.45, 0.5))  # draw 0, draw 1


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def grid(dev) -> int:
    "G: the persistent inverse kernel's grid (two blocks per CU)"
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def fft_dev(dev) -> torch.device:
    "where the float64 colorize runs: the device, if torch's float64 FFT there agrees with the host's; else the host, in chunks"
    x = torch.randn(2, 4, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    try:
        y = torch.fft.irfftn(torch.fft.rfftn(x.to(dev), dim=(-3, -2, -1)) * 1.5, s=(4, 16, 16), dim=(-3, -2, -1)).cpu()
    except RuntimeError:
        return torch.device("cpu")
    return dev if (y - x * 1.5).abs().max().item() < 1e-12 else torch.device("cpu")


def resolve(name: str, G: int) -> tuple[int, int, torch.dtype, int]:
    "(batch, d1, dtype, planes) of a case; a plane count d1 does not divide (a grid of an unusual CU count) rounds up to whole samples"
    planes_of, d1, dtype = CASES[name]
    batch = -(-planes_of(G, d1) // d1)
    return batch, d1, dtype, batch * d1


def seeds_of(name: str, batch: int) -> list[int]:
    base = 10_000 * (1 + sorted(CASES).index(name))
    return [base + 3 * i for i in range(batch)]


def stats() -> tuple[int, int]:
    lib = _hip.load()
    return lib.skr_stat(b"colored_inv128_launches"), lib.skr_stat(b"colored_inv128_ticketed")


def weights64(unit, exponent: float, device) -> torch.Tensor:
    "ON.colorize's spectral weights, computed as it computes them (on the host), then moved"
    grid = ON.radial_freq_grid(unit)
    clip = 0.5 / max(sum(unit) / len(unit), 4.0)
    return (torch.clamp(grid, min=clip) ** (-exponent / 2.0)).to(device=device, dtype=torch.float64)


def colorize64(white: torch.Tensor, exponent: float, energy: float | None, fft_dev: torch.device) -> torch.Tensor:
    """ON.colorize (oracle/skr_oracle/noise.py) for a batch of (d1, 128, 128) units in float64: white [B, d1, H, W] -> [B, d1, H, W]
    on white's device; unbiased std per sample, the cstd > 1e-8 rule and the energy rule"""
    B, unit = white.shape[0], tuple(white.shape[1:])
    out = torch.empty(white.shape, dtype=torch.float64, device=white.device)
    dims = tuple(range(-len(unit), 0))
    w8 = weights64(unit, exponent, fft_dev) if exponent != 0.0 else None
    for s0 in range(0, B, CHUNK):
        w = white[s0 : s0 + CHUNK].to(device=fft_dev, dtype=torch.float64)
        b = w.shape[0]
        wstd = w.reshape(b, -1).std(dim=1)
        if exponent == 0.0:
            if energy is None:
                col = w
            else:
                col = w * torch.where(wstd < 1e-8, torch.ones_like(wstd), energy / wstd).view(b, 1, 1, 1)
        else:
            col = torch.fft.irfftn(torch.fft.rfftn(w, dim=dims) * w8, s=unit, dim=dims)
            cstd = col.reshape(b, -1).std(dim=1)
            target = wstd if energy is None else torch.full_like(cstd, energy)
            col = col * torch.where(cstd > 1e-8, target / cstd, torch.ones_like(cstd)).view(b, 1, 1, 1)
        out[s0 : s0 + b] = col.to(white.device)
    return out


def ulp16(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    "one unit in the last place of `dtype` at |ref| (fp16: subnormal spacing below 2^-14)"
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0**emin)))
    return torch.exp2(e - mant)


def assert_every_sample(got: torch.Tensor, ref: torch.Tensor, what: str) -> float:
    """the per-sample bar; returns (and records) the measured worst value: relative inf-norm error (fp32), or how far beyond one
    last-place unit an element went, as a fraction of its sample's max |ref| (16-bit)"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    B = got.shape[0]
    assert bool(torch.isfinite(got).all()), (what, "non-finite output", int((~torch.isfinite(got)).sum()))
    g = got.to(torch.float64)
    diff = (g - ref).abs()
    scale = ref.abs().reshape(B, -1).amax(dim=1)
    family = "colored whole batch " + str(got.dtype).replace("torch.", "")
    if got.dtype == torch.float32:
        err = diff.reshape(B, -1).amax(dim=1) / scale
        worst = note_margin(family, "per-sample rel inf-norm error vs float64", err.max().item(), COLORED_TOL)
        bad = (err > COLORED_TOL).nonzero().flatten().tolist()
        assert not bad, (what, "samples over the bar", bad[:16], err.max().item())
        return worst
    ulp = ulp16(ref, got.dtype)
    beyond = ((diff - ulp).clamp_min(0).reshape(B, -1).amax(dim=1) / scale)
    big = ref.abs() >= 1e-3 * scale.view(B, *([1] * (ref.dim() - 1)))  # (near zero a last place is far below the fp32 noise of the transform)
    note_margin(family, "max |diff| in last-place units of the reference (elements >= 1e-3 max|ref|)", (diff[big] / ulp[big]).max().item(), None)
    worst = note_margin(family, "per-sample max (|diff| - 1 ulp) / max|ref|", beyond.max().item(), ADDITIVE_16)
    bad = (beyond > ADDITIVE_16).nonzero().flatten().tolist()
    assert not bad, (what, "samples over the bar", bad[:16], beyond.max().item())
    return worst


def spot_check_white(white: torch.Tensor, seeds: list[int], n: int) -> None:
    "Random's draw n is the Philox specification's stream n * 256 (three samples; the suite's 4e-6)"
    B, unit = white.shape[0], tuple(white.shape[1:])
    for j in sorted({0, B // 2, B - 1}):
        spec = torch.from_numpy(ON.philox_normal(seeds[j], n * 256, math.prod(unit))).reshape(unit)
        assert (white[j].cpu().double() - spec).abs().max().item() < 4e-6, (j, n)


def white_draws(unit, seeds, count: int) -> list[torch.Tensor]:
    g = PN.BatchTensorNoise.from_batch_inputs(PN.Random, unit, seeds, dtype=torch.float32)
    return [g.generate(None) for _ in range(count)]


def test_float64_colorize_is_the_oracle(dev, fft_dev):
    "the batched float64 restatement equals ON.colorize run on the host in float64, on two samples, within 1e-12"
    unit, seeds = (16, H, W), [77, 78, 79]
    white = white_draws(unit, seeds, 1)[0]
    cases = [(0.25, None), (-1.4, None), (1.7, 2.5), (0.0, -1.5)]
    for exponent, energy in cases:
        got = colorize64(white, exponent, energy, fft_dev)
        for j in (0, 2):
            want = ON.colorize(white[j].cpu().double(), exponent, energy)
            err = ((got[j].cpu() - want).abs().max() / want.abs().max()).item()
            assert err < 1e-12, (exponent, energy, j, err)


@pytest.mark.parametrize("name", list(CASES))
def test_every_sample_against_float64(name, dev, grid, fft_dev):
    batch, d1, dtype, planes = resolve(name, grid)
    unit, seeds = (d1, H, W), seeds_of(name, batch)
    props = PN.ColoredProps()
    gen = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, unit, seeds, props=props, dtype=dtype)
    whites = white_draws(unit, seeds, len(STEPS))
    kw = dict(color_start=props.color_start, color_end=props.color_end, color_curve=props.color_curve)
    for n, step in enumerate(STEPS):
        launches, ticketed = stats()
        got = gen.generate(step)
        torch.cuda.synchronize()
        launches2, ticketed2 = stats()
        assert launches2 - launches == 1, (name, "colored_inverse128 did not run", launches2 - launches)
        assert ticketed2 - ticketed == (1 if planes > 2 * grid else 0), (name, planes, grid, ticketed2 - ticketed)
        spot_check_white(whites[n], seeds, n)
        ref = colorize64(whites[n], ON.colored_exponent(step, **kw), None, fft_dev)
        assert_every_sample(got, ref, f"{name} ({batch} x {unit} {dtype}, {planes} planes, G = {grid}) draw {n}")
        del got, ref
    torch.cuda.empty_cache()


@pytest.mark.parametrize(("props", "step"), [(PN.ColoredProps(energy=2.5, color_start=1.5, color_end=-3, color_curve=0), Step(0.45, 0.5)), (PN.ColoredProps(energy=-1.5, color_start=0.0), None)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cfg3c_with_energy_against_float64(props, step, dtype, dev, grid, fft_dev):
    batch, d1 = 256, 16
    unit, seeds = (d1, H, W), [50_000 + i for i in range(batch)]
    gen = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, unit, seeds, props=props, dtype=dtype)
    launches, ticketed = stats()
    got = gen.generate(step)
    torch.cuda.synchronize()
    assert stats() == (launches + 1, ticketed + (1 if batch * d1 > 2 * grid else 0))
    white = white_draws(unit, seeds, 1)[0]
    spot_check_white(white, seeds, 0)
    exponent = ON.colored_exponent(step, color_start=props.color_start, color_end=props.color_end, color_curve=props.color_curve)
    ref = colorize64(white, exponent, props.energy, fft_dev)
    assert_every_sample(got, ref, f"cfg3c {props} {step}")
    if dtype == torch.float32:
        std = got.double().reshape(batch, -1).std(dim=1)
        assert (std - abs(props.energy)).abs().max().item() < 1e-4


# ---- NaN-filled buffers owned by the test -------------------------------------------------------------------------------
def colored_workspaces(batch: int, d1: int, dev) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, int]:
    "the workspaces PN.Colored._batch allocates for (d1, 128, 128) units: spectrum, scratch, partials (4 * batch * slots doubles), slots"
    unit, half = d1 * H * W, d1 * H * (W // 2 + 1)
    slots = max(256, -(-(unit // W) // max(2, 2 * (256 // W))))
    return (torch.empty(batch * half, dtype=torch.complex64, device=dev), torch.empty(batch * unit, dtype=torch.float32, device=dev),
            torch.empty(4 * batch * slots, dtype=torch.float64, device=dev), slots)  # fmt: skip


def call_colored(out, spec, scratch, partials, slots, seeds_dev, stream: int, d1: int, exponent: float) -> None:
    lib = _hip.load()
    status = lib.skr_noise_colored(
        out.data_ptr(), _hip.DTYPE_CODE[out.dtype], spec.data_ptr(), scratch.data_ptr(), partials.data_ptr(), slots, seeds_dev.data_ptr(), stream,
        out.shape[0], d1, H, W, float(exponent), 0, 0.0, _hip.current_stream_ptr(out.device),
    )  # fmt: skip
    _hip.check(status, "skr_noise_colored")


@pytest.mark.parametrize("name", ["cfg3c_fp32", "2G_plus_d1_d1=8"])
def test_no_element_is_left_unwritten(name, dev, grid, fft_dev):
    """out, spectrum and scratch filled with NaN, the partials too except their trailing 2 * batch doubles (the factors, the plane
    ticket and the arrival counters: DESIGN.md), which hold what an earlier draw on the same workspaces left there -- never values
    written by hand: a ticket past 2^31 would send the inverse kernel's loop outside its buffers"""
    batch, d1, dtype, planes = resolve(name, grid)
    unit, seeds = (d1, H, W), seeds_of(name, batch)
    seeds_dev = PN.seeds_tensor(seeds, dev)
    spec, scratch, partials, slots = colored_workspaces(batch, d1, dev)
    exponent = ON.colored_exponent(None)
    out = torch.empty((batch, *unit), dtype=dtype, device=dev)
    call_colored(out, spec, scratch, partials, slots, seeds_dev, 7 * 256, d1, 1.3)  # the earlier draw: another stream, another exponent
    torch.cuda.synchronize()
    nan = float("nan")
    out.fill_(nan)
    spec.fill_(complex(nan, nan))
    scratch.fill_(nan)
    partials[: partials.numel() - 2 * batch].fill_(nan)
    launches, ticketed = stats()
    call_colored(out, spec, scratch, partials, slots, seeds_dev, 0, d1, exponent)
    torch.cuda.synchronize()
    assert stats() == (launches + 1, ticketed + (1 if planes > 2 * grid else 0))
    white = white_draws(unit, seeds, 1)[0]
    assert_every_sample(out, colorize64(white, exponent, None, fft_dev), f"{name} into NaN-filled buffers")
    gen = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, unit, seeds, props=PN.ColoredProps(), dtype=dtype)
    assert torch.equal(out, gen.generate(None))


# ---- the host-selected variants, each in a fresh process ----------------------------------------------------------------
CHILD = """
import json, sys
sys.path[:0] = [{root!r}, {oracle!r}]
import torch
from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.pytorch import noise as PN
_hip.load()
jobs = json.loads(sys.argv[1])
out = {{}}
lib = _hip.load()
for key, batch, d1, dtype, seeds in jobs:
    gen = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, (d1, 128, 128), seeds, props=PN.ColoredProps(), dtype=getattr(torch, dtype))
    out[key] = [gen.generate(None).cpu(), gen.generate(Step(0.45, 0.5)).cpu()]
torch.cuda.synchronize()
out["stats"] = (lib.skr_stat(b"colored_inv128_launches"), lib.skr_stat(b"colored_inv128_ticketed"))
torch.save(out, sys.argv[2])
"""
VARIANT_CASES = ["cfg3c_fp32", "cfg3c_bf16", "2G_plus_d1_d1=8"]
# variant: (environment, bitwise equal to the default process)
VARIANTS = {
    # the same per-plane arithmetic and the same factors, only a different deal of planes to blocks / another grid
    "static_deal": ({"SKR_COLORED_INV_STATIC": "1"}, True),
    "one_block_per_cu": ({"SKR_COLORED_INV_BLOCKS": "1"}, True),
    "eight_blocks_per_cu": ({"SKR_COLORED_INV_BLOCKS": "8"}, True),
    # colored_factors sums the same slots in the same fixed order with the same rescale_factor as the last outer-axis block does
    "factors_kernel": ({"SKR_COLORED_FACTORS_KERNEL": "1"}, True),
    # colored_plane<1>: another inverse transform (the LDS plane kernel's own radix passes), so other fp32 roundings
    "old_inverse": ({"SKR_COLORED_OLD_INVERSE": "1"}, False),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_selected_variant(variant, dev, grid, fft_dev, tmp_path):
    env_add, bitwise = VARIANTS[variant]
    jobs = []
    for name in VARIANT_CASES:
        batch, d1, dtype, _ = resolve(name, grid)
        jobs.append((name, batch, d1, str(dtype).replace("torch.", ""), seeds_of(name, batch)))
    script = tmp_path / "child.py"
    script.write_text(CHILD.format(root=ROOT, oracle=os.path.join(ROOT, "oracle")))
    saved = tmp_path / "out.pt"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SKR_COLORED_")}
    env.update(env_add)
    proc = subprocess.run([sys.executable, str(script), json.dumps(jobs), str(saved)], env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, (variant, proc.returncode, proc.stderr[-3000:])  # (a signal shows as a negative code: the test ends here)
    child = torch.load(saved)
    launches, ticketed = child["stats"]
    if variant == "old_inverse":
        assert launches == 0 and ticketed == 0, child["stats"]
    else:
        assert launches == 2 * len(jobs), child["stats"]
        if variant == "static_deal":
            assert ticketed == 0, child["stats"]
    kw = dict(color_start=PN.ColoredProps().color_start, color_end=PN.ColoredProps().color_end, color_curve=PN.ColoredProps().color_curve)
    for name, batch, d1, dtype, seeds in jobs:
        gen = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, (d1, H, W), seeds, props=PN.ColoredProps(), dtype=getattr(torch, dtype))
        whites = white_draws((d1, H, W), seeds, len(STEPS))
        for n, step in enumerate(STEPS):
            default = gen.generate(step)
            got = child[name][n].to(dev)
            same = torch.equal(got, default)
            note_margin("colored whole batch variant " + variant, "bitwise equal to the default process (1 = yes)", float(same), None)
            if bitwise:
                assert same, (variant, name, n, int((got != default).sum()))
            ref = colorize64(whites[n], ON.colored_exponent(step, **kw), None, fft_dev)
            assert_every_sample(got, ref, f"{variant}: {name} draw {n}")
            del default, got, ref
        torch.cuda.empty_cache()
