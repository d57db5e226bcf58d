import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run by the driver with -m gpu)")


def pytest_collection_modifyitems(config, items):
    try:
        import torch

        have_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        have_gpu = False
    if have_gpu:
        return
    skip = pytest.mark.skip(reason="no HIP device in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(autouse=True)
def _reproducible_global_rngs(request):
    """Every test starts from global RNG states derived from its own id, so the few inputs drawn without an explicit generator do
    not depend on which tests ran before, on the process (str hashes) or on the run."""
    import random
    import zlib

    import torch

    seed = zlib.crc32(request.node.nodeid.encode())
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)  # (seeds the HIP generators too when a device is present)
    yield


# ---- measured parity margins --------------------------------------------------------------------------------------------
# With SKR_PARITY_MARGINS=<file> every parity comparison of the GPU suite appends what it MEASURED (one JSON line: test id,
# family, measure, value, bar) -- tools/summarize_margins.py condenses the file into profiles/r04_parity_margins.txt, the
# record the tolerances written in the tests are justified against.
_current_test = [""]


@pytest.fixture(autouse=True)
def _margin_context(request):
    _current_test[0] = request.node.nodeid
    yield


def note_margin(family: str, measure: str, value: float, bar: float | None = None) -> float:
    path = os.environ.get("SKR_PARITY_MARGINS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"test": _current_test[0], "family": family, "measure": measure, "value": float(value), "bar": bar}) + "\n")
    return value


@pytest.fixture(scope="session")
def kats():
    return json.load(open(os.path.join(GOLDEN, "reference_kats.json")))


@pytest.fixture(scope="session")
def tables():
    return json.load(open(os.path.join(GOLDEN, "tables.json")))


# ---- host numerics: MKL's code branch -------------------------------------------------------------------------------------
# torch's CPU FFT and vector math run on MKL, whose last bits differ between its AVX-512 branch (Intel CPUs, where the fixtures were
# recorded) and the generic branch it takes on other CPUs.  mkl_generic.npz holds the reference's own results recorded on the generic
# branch (tools/make_mkl_overlay.py) for the cases a non-Intel host reproduces from that recording -- the FFT-based noise -- and a
# canary transform recorded on both branches.  load_npz hands those values over, bit for bit, on a host whose canary matches the
# generic branch; every other host gets the fixtures as recorded.
MKL_GENERIC = "mkl_generic.npz"
_mkl_overlay: list = []


def host_fft_canary() -> np.ndarray:
    "a real 3-D FFT of fixed, RNG-free input on this host's torch CPU path"
    import torch

    x = (torch.arange(4 * 16 * 16, dtype=torch.float64) * 0.6180339887498949).remainder(1.0).to(torch.float32).reshape(4, 16, 16)
    return torch.view_as_real(torch.fft.rfftn(x)).numpy()


def host_mkl_generic() -> bool:
    "this host's MKL takes the generic branch: its canary transform matches that branch's recording (and not the fixtures' own)"
    if not _mkl_overlay:
        with np.load(os.path.join(GOLDEN, MKL_GENERIC)) as z:
            blob = {k: z[k] for k in z.files}
        generic = np.array_equal(host_fft_canary(), blob["canary/generic"]) and not np.array_equal(blob["canary/generic"], blob["canary/recorded"])
        _mkl_overlay.append((generic, {k: v for k, v in blob.items() if "::" in k} if generic else {}))
    return _mkl_overlay[0][0]


def mkl_overlay() -> dict:
    "{'<fixture file>::<key>': generic-branch value} when this host's MKL takes the generic branch, else {}"
    host_mkl_generic()
    return _mkl_overlay[0][1]


def load_npz(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, name)) as z:
        blob = {k: z[k] for k in z.files}
    for key, value in mkl_overlay().items():
        fname, _, k = key.partition("::")
        if fname == name:
            assert k in blob, key
            blob[k] = value
    return blob


def eq_nan(a, b) -> bool:
    return np.array_equal(np.asarray(a, dtype=float), np.asarray(b, dtype=float), equal_nan=True)
