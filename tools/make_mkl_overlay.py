#!/usr/bin/env python3
"""Generate tests/golden/mkl_generic.npz (build container only): the reference's results on MKL's generic code branch.

torch's CPU FFT and vector math run on MKL.  On Intel CPUs MKL takes its AVX-512 branch, where tests/golden/* were recorded; on other
CPUs it takes a generic branch (the one MKL_CBWR=COMPATIBLE selects on Intel) whose last bits differ.  This re-runs
tools/make_golden.py with MKL_CBWR=COMPATIBLE into a temporary directory and stores, for the fixtures in FILES, every value that
differs from the committed one, keyed '<file>::<key>', plus a canary transform (tests/conftest.py::host_fft_canary) on both branches.
tests/conftest.py::load_npz serves these values on a host whose canary matches the generic branch.

FILES are the cases a non-Intel host reproduces from the generic-branch recording: the FFT-based noise (Colored, N-D colorize).
Values that go through MKL's vector sqrt are not: its last bits differ between Intel's generic branch and other CPUs' (an AMD EPYC
host reproduces the AVX-512 recording of common_api.json's spowf and steps_extra2.npz's SPC power cases, and neither recording of
steps_sweep.npz's SPC power blends, which its replay then leaves out: tests/test_oracle_golden.py).

usage: python tools/make_mkl_overlay.py
"""

from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("noise.npz", "colorize_nd.npz")


def canary(env: dict) -> np.ndarray:
    "host_fft_canary in a fresh process (MKL reads MKL_CBWR once, when it starts)"
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "canary.npy")
        code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import numpy, conftest; numpy.save({path!r}, conftest.host_fft_canary())"
        subprocess.run([sys.executable, "-c", code], env=env, check=True)
        return np.load(path)


def same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")


def main() -> None:
    generic = {**os.environ, "MKL_CBWR": "COMPATIBLE"}
    recorded = {k: v for k, v in os.environ.items() if k != "MKL_CBWR"}
    blob = {"canary/recorded": canary(recorded), "canary/generic": canary(generic)}
    assert not same(blob["canary/recorded"], blob["canary/generic"]), "this host's MKL takes the generic branch already: run on an Intel CPU"
    with tempfile.TemporaryDirectory() as out:
        subprocess.run([sys.executable, os.path.join(HERE, "make_golden.py")], env={**generic, "SKR_GOLDEN_OUT": out}, check=True, stdout=subprocess.DEVNULL)
        for name in FILES:
            with np.load(os.path.join(GOLDEN, name)) as a, np.load(os.path.join(out, name)) as b:
                assert sorted(a.files) == sorted(b.files), name
                for k in a.files:
                    if not same(a[k], b[k]):
                        blob[f"{name}::{k}"] = b[k]
    np.savez_compressed(os.path.join(GOLDEN, "mkl_generic.npz"), **blob)
    print(f"mkl_generic.npz: {len(blob) - 2} values", sorted(blob))


if __name__ == "__main__":
    main()
