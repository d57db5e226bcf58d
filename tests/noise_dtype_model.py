#!/usr/bin/env python3
"""How many elements a fused multiply-convert store would get wrong: the host model behind tests/test_noise_dtype_contract_gpu.py (no GPU).

    python tests/noise_dtype_model.py [--elements N]

The generators' contract is fp32 arithmetic, then one rounding to nearest even to the output dtype.  gfx950 has an instruction that
multiplies two fp32 numbers and rounds the EXACT product to fp16 (v_fma_mixlo_f16); a store `(fp16)(a * b)` compiled to it differs from
the contract exactly where fl32(a * b) is an fp16 tie and a * b is not.  The product of two fp32 numbers is exact in float64, and numpy
narrows float64 to float16 in one rounding, so
    fused     float16(float64(a) * float64(b))
    contract  float16(float32(float64(a) * float64(b)))
and the count of elements on which they differ is the expected number of failures of one test id on a library with such a store.
Last operations of the scalar stores (csrc): Random / Offset `r * cos(t)` of Box-Muller (Offset adds the offset behind it: no product
in front of the conversion), Pyramid `scratch * inv`, Colored `real * factor`, Brownian `scale * (to - from)`."""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from skr_oracle import noise as ON  # noqa: E402


def fused_differs(a: np.ndarray, b) -> int:
    p = a.astype(np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)  # exact: 48 bits at most
    with np.errstate(over="ignore"):
        once, twice = p.astype(np.float16), p.astype(np.float32).astype(np.float16)
    return int((once.view(np.uint16) != twice.view(np.uint16)).sum())


def box_muller_factors(n: int, seed: int = 1000, stream: int = 7 * 256):
    "(r, cos / sin) of the first n normals of (seed, stream), as oracle.box_muller forms them"
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([(blocks & 0xFFFFFFFF).astype(np.uint32), (blocks >> np.uint64(32)).astype(np.uint32), np.full(blocks.shape, stream, np.uint32), np.zeros(blocks.shape, np.uint32)], -1)
    x = ON.philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)).astype(np.float32) * np.float32(2.0**-32) + np.float32(2.0**-33)
    x = np.minimum(x, np.float32(1.0))
    r, t = np.empty(x.shape, np.float32), np.empty(x.shape, np.float32)
    for a, b in ((0, 1), (2, 3)):
        r[..., a] = r[..., b] = np.sqrt(np.float32(-2.0) * np.log(x[..., a])).astype(np.float32)
        th = (np.float32(2 * np.pi) * x[..., b]).astype(np.float32)
        t[..., a], t[..., b] = np.cos(th), np.sin(th)
    return r.reshape(-1)[:n], t.reshape(-1)[:n]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=1 << 21)
    n = ap.parse_args().elements
    r, t = box_muller_factors(n)
    z = (r * t).astype(np.float32)
    print(f"elements differing between the fused store and the contract, of {n} (n * 2^-14 = {n / 16384:.0f}):")
    print(f"  r * cos(t), r * sin(t)        Random, generic kernel            {fused_differs(r, t)}")
    print(f"  first 65536 of them                                             {fused_differs(r[:65536], t[:65536])}")
    for what, scale in (("z * 1 (a scale of exactly one)", 1.0), ("z * 0.9173 (Pyramid: scratch * inv)", 0.9173), ("z * 1.3071e-3 (Colored: real * factor)", 1.3071e-3),
                        ("z * 4.4721 (Brownian: scale * (to - from), 20 steps)", 20.0**0.5)):  # fmt: skip
        print(f"  {what:<62}  {fused_differs(z, np.float32(scale))}")
    print("  (bf16: gfx950 has no fused multiply-convert to bf16, a bf16 store is v_cvt_pk_bf16_f32 of the fp32 value: 0 expected)")


if __name__ == "__main__":
    main()
