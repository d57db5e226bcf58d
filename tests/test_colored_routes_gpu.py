"""Every dispatch arm of the colored-noise launchers in every output dtype.

The launchers of csrc/skr_colored.hip pick a kernel instantiation per (route, plane form, output dtype).  The oracle tests of
test_noise_gpu.py pin every route in fp32; what they cannot see is a launcher that picks the wrong instantiation for another dtype.
So each unit below -- the smallest that reaches its arm -- is drawn in bf16, fp16, fp32 and float64 with the same seeds, and the
other three are held to the fp32 draw:
  float64      relative inf-norm error below 1e-5 (the bar of every fp32 generator comparison of the suite)
  bf16 / fp16  every element has the bits of the fp32 value rounded once, to nearest even (bit_model.round_to / same_bits): the three
               instantiations of a route run the same fp32 arithmetic and differ in their store alone (csrc/skr_pack.h; at 2^21 elements
               per store path: tests/test_noise_dtype_contract_gpu.py)
and every draw is finite with a std within 0.05 of 1.  No draw may reach hipFFT, and the persistent 128 x 128 inverse kernel runs
for the units with 128 x 128 planes under a leading axis and for no other.
(The std bar is the white noise's own at the smallest units: 3 samples of 128 elements spread by 3.6 %.  With these seeds the
fp32 oracle's draws of every unit sit within 0.035 of 1, so the bar holds the rescale and not the luck of the sample.)"""

import bit_model as BM
import pytest
import torch

from skrample_amd import _hip
from skrample_amd.common import Step
from skrample_amd.pytorch import noise as PN

pytestmark = pytest.mark.gpu

SEEDS = [41, 42, 43]

ARMS = {
    "fused planes (generic / 64 / 128 forms, 2-D and 3-D)": [(8, 16), (64, 64), (128, 128), (2, 8, 16), (2, 64, 64), (2, 128, 128)],
    "outer-axis register kernel, every d1": [(4, 8, 16), (8, 8, 16), (16, 8, 16)],
    "mixed planes (512 / 1024 threads, run-time and compile-time sides, 2-D and 3-D)": [(12, 24), (2, 12, 24), (96, 96), (2, 96, 96), (160, 160), (192, 192), (2, 192, 192)],
    "separate passes": [(128, 256), (2, 128, 256), (4, 128, 256), (8, 128, 256), (32, 8, 16)],
    "colored_planes through skr_noise_colored_any": [(3, 8, 16), (3, 64, 64), (3, 128, 128), (3, 12, 24), (3, 160, 160), (2, 3, 8, 16)],
}
UNITS = [u for units in ARMS.values() for u in units]
INVERSE128 = {(2, 128, 128), (3, 128, 128)}


@pytest.mark.parametrize("unit", UNITS, ids=lambda u: "x".join(map(str, u)))
def test_every_dtype_of_every_route_agrees_with_the_fp32_draw(unit):
    lib = _hip.load()
    before = lib.skr_stat(b"hipfft_execs"), lib.skr_stat(b"colored_inv128_launches")
    draws = {}
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        g = PN.BatchTensorNoise.from_batch_inputs(PN.Colored, unit, SEEDS, props=PN.ColoredProps(), dtype=dtype)
        draws[dtype] = [g.generate(st).clone() for st in (None, Step(0.3, 0.4))]
        assert all(d.dtype == dtype and d.shape == (len(SEEDS), *unit) for d in draws[dtype])
    torch.cuda.synchronize()
    after = lib.skr_stat(b"hipfft_execs"), lib.skr_stat(b"colored_inv128_launches")
    assert after[0] == before[0], "a colored draw went to hipFFT"
    assert (after[1] > before[1]) == (unit in INVERSE128), (unit, before, after)

    for n, want in enumerate(draws[torch.float32]):
        want = want.cpu().double()
        for dtype, got in draws.items():
            got = got[n].cpu().double()
            assert torch.isfinite(got).all(), (unit, dtype, n)
            std = got.std().item()
            assert abs(std - 1.0) < 0.05, (unit, dtype, n, std)
            diff = (got - want).abs()
            if dtype == torch.float64:
                err = (diff.max() / want.abs().max()).item()
                print(f"{unit} float64 draw {n}: rel inf-norm {err:.3g}")
                assert err < 1e-5, (unit, n, err)
            elif dtype in (torch.bfloat16, torch.float16):
                rounded = BM.round_to(dtype, draws[torch.float32][n].cpu().numpy().reshape(-1))
                print(f"{unit} {dtype} draw {n}: {int(BM.differing(draws[dtype][n].cpu().reshape(-1), rounded).sum())} of {rounded.numel()} elements differ from the rounded fp32 draw")
                BM.same_bits(draws[dtype][n].cpu().reshape(-1), rounded, what=f"{unit} {dtype} draw {n}")
