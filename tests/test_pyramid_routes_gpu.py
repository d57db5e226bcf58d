"""Every pass-1 form of the Pyramid launchers, and both any-shape entries, in every output dtype.

skr_noise_pyramid picks one of five instantiations of pyramid_pass1 by the plane's shape (choose_pyramid_route, csrc/skr_launch.h; the
table is in DESIGN.md section 4.3), and the Python layer takes skr_noise_pyramid_any for the shapes it refuses and skr_noise_pyramid_nd
for resized axes that are not the trailing ones.  Each unit below is the smallest that reaches its arm.  It is drawn twice with three
seeds in fp32, float64, bf16 and fp16:
  fp32         against the oracle (pyramid_reference of test_noise_gpu.py) at the suite's PYRAMID_TOL, per-sample std within 1e-4 of 1
  float64      relative inf-norm error against the fp32 draw below 1e-5 (the bar of every fp32 generator comparison of the suite)
  bf16 / fp16  every element within one unit in the last place of its format of the fp32 value (8 / 11 significant bits):
               |a - b| <= 2^-7 (2^-10) max(|a|, |b|) + 1e-6
(the generators compute in fp32 whatever the output: pass 2 rounds the same fp32 quotient to the output dtype) and "any_shape" is in
the generator's state for exactly the two units the LDS entry refuses."""

import pytest
import torch

from skrample_amd.pytorch import noise as PN
from test_noise_gpu import PYRAMID_TOL, pyramid_reference, rel

pytestmark = pytest.mark.gpu

SEEDS = [41, 42, 43]
ULP = {torch.bfloat16: 2.0**-7, torch.float16: 2.0**-10}

ARMS = {  # (unit, props)
    "generic": [((1, 16, 16), {}), ((2, 16, 16), {}), ((8, 64), dict(dims=(-1,)))],
    "generic with the LDS opt-in": [((1, 200, 300), {})],
    "strip 256": [((1, 96, 128), {})],
    "strip 512": [((1, 192, 128), {})],
    "strip 1024 without UNI (LDS opt-in)": [((1, 384, 128), {})],
    "UNI": [((1, 192, 256), {}), ((1, 96, 512), {}), ((1, 256, 256), {})],
    "refused by the LDS entry: skr_noise_pyramid_any": [((3, 30, 90), {}), ((1, 400, 400), {})],
    "an axis pair: skr_noise_pyramid_nd": [((8, 3, 16), dict(dims=(0, 2)))],
}
CASES = [c for cases in ARMS.values() for c in cases]
FALLBACK = {(3, 30, 90), (1, 400, 400)}


@pytest.mark.parametrize(("unit", "kw"), CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "-".join(f"{k}{v}" for k, v in v.items()) or "trailing")
def test_every_dtype_of_every_route(unit, kw):
    props = PN.PyramidProps(**kw)
    draws = {}
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.float16):
        g = PN.BatchTensorNoise.from_batch_inputs(PN.Pyramid, unit, SEEDS, props=props, dtype=dtype)
        draws[dtype] = [g.generate(None).cpu() for _ in range(2)]
        assert all(d.dtype == dtype and d.shape == (len(SEEDS), *unit) for d in draws[dtype])
        assert ("any_shape" in g._state) == (unit in FALLBACK), (unit, dtype, sorted(map(str, g._state)))

    for n, got in enumerate(draws[torch.float32]):
        ref = torch.stack([pyramid_reference(unit, s, n * 256, **kw) for s in SEEDS])
        err = rel(got, ref, "pyramid (every route)", PYRAMID_TOL)
        spread = (got.reshape(len(SEEDS), -1).double().std(dim=1) - 1).abs().max().item()
        print(f"{unit} fp32 draw {n}: rel inf-norm vs the oracle {err:.3g}, per-sample std off 1 by {spread:.3g}")
        assert err < PYRAMID_TOL, (unit, kw, n, err)
        assert spread < 1e-4, (unit, kw, n, spread)

    for n, want in enumerate(draws[torch.float32]):
        want = want.double()
        for dtype, got in draws.items():
            got = got[n].double()
            assert torch.isfinite(got).all(), (unit, dtype, n)
            diff = (got - want).abs()
            if dtype == torch.float64:
                err = (diff.max() / want.abs().max()).item()
                print(f"{unit} float64 draw {n}: rel inf-norm {err:.3g}")
                assert err < 1e-5, (unit, n, err)
            elif dtype in ULP:
                worst = (diff / (torch.maximum(got.abs(), want.abs()) + 1e-30)).max().item() / ULP[dtype]
                print(f"{unit} {dtype} draw {n}: worst difference {worst:.3g} units in the last place")
                assert (diff <= ULP[dtype] * torch.maximum(got.abs(), want.abs()) + 1e-6).all(), (unit, dtype, n, worst)
