"""Per-sample schedule slots without a GPU: the host-side validation of `CapturedLoop.__call__`, the index arithmetic and the
[steps, batch] timestep assembly (on stub rows and loops -- nothing here enqueues device work), and the new export at the C boundary."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
from conftest import ROOT

from skrample_amd import _hip
from skrample_amd.graphs import CapturedLoop, capture_sampling_loop

NAME = "skr_step_launch_indexed_per_sample"


class StubRows:
    "what CapturedLoop reads of an _hip.IndexedRows, on the host"

    def __init__(self, slots: int, length: int, batch: int | None):
        self.slots, self.length, self.batch = slots, length, batch
        self.index_dev = torch.zeros(1, dtype=torch.int32)
        self.sample_index_dev = torch.zeros(batch, dtype=torch.int32) if batch is not None else None

    sample_indices = _hip.IndexedRows.sample_indices
    select = _hip.IndexedRows.select


class StubGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


def stub_loop(batch=4, slots=3, length=7, steps=5, per_sample=True, filled=(0, 1)):
    x = torch.zeros(batch, 2)
    times = torch.arange(steps, dtype=torch.float32)
    sample_times = times.unsqueeze(1).repeat(1, batch) if per_sample else None
    loop = CapturedLoop(StubGraph(), x.clone(), x.clone(), None, StubRows(slots, length, batch if per_sample else None), None, times, sample_times)
    for k in filled:
        loop._filled.add(k)
        loop._times[k] = times + 100.0 * k
    return loop


def test_slot_vector_validation_happens_before_anything_is_enqueued():
    loop = stub_loop()
    x = torch.ones(4, 2)
    for bad, message in (([0, 1, 0], "3 slots for a captured batch of 4"), ([0, 1, 0, 1, 0], "5 slots"), ([0, 1, 3, 0], "slot 3 outside 0..2"), ([0, -1, 0, 0], "slot -1 outside"),
                         ([0, 2, 0, 0], r"schedule slot 2 has never been loaded: call retarget\(wrapper, slot=2\) first"), (torch.tensor([0.0, 1.0, 0.0, 1.0]), "CPU integer tensor"),
                         (torch.zeros(2, 2, dtype=torch.int64), "CPU integer tensor")):  # fmt: skip
        with pytest.raises(ValueError, match=message):
            loop(x, slot=bad)
    assert loop.graph.replays == 0 and not loop.static_in.any() and not loop.rows.sample_index_dev.any()  # nothing copied, nothing published
    out = loop(x, slot=(1, 0, 0, 1))
    assert loop.graph.replays == 1 and loop.static_in.eq(1).all() and out.shape == x.shape


def test_sequence_on_a_loop_captured_without_per_sample():
    loop = stub_loop(per_sample=False)
    assert not loop.per_sample
    with pytest.raises(ValueError, match="per_sample=True"):
        loop(torch.ones(4, 2), slot=[0, 1, 0, 1])
    assert loop.graph.replays == 0
    loop(torch.ones(4, 2), slot=1)  # the int form is what it always was
    assert loop.rows.index_dev.item() == 7 and loop.graph.replays == 1


def test_per_sample_needs_indexed():
    with pytest.raises(ValueError, match="indexed=True"):
        capture_sampling_loop(object(), lambda x, t: x, torch.zeros(2, 4), 3, per_sample=True)


def test_index_arithmetic():
    "sample b reads row slot[b] * length + position in the loop"
    loop = stub_loop(batch=4, slots=3, length=7)
    loop(torch.ones(4, 2), slot=[1, 0, 0, 1])
    assert loop.rows.sample_index_dev.dtype == torch.int32 and loop.rows.sample_index_dev.tolist() == [7, 0, 0, 7]
    loop(torch.ones(4, 2), slot=torch.tensor([0, 1, 1, 0], dtype=torch.int16))
    assert loop.rows.sample_index_dev.tolist() == [0, 7, 7, 0]
    loop(torch.ones(4, 2), slot=1)  # an int means every sample, on both indices
    assert loop.rows.sample_index_dev.tolist() == [7] * 4 and loop.rows.index_dev.item() == 7
    rows = StubRows(slots=256, length=30, batch=256)
    assert rows.sample_indices(range(256)).tolist() == [30 * k for k in range(256)]


def test_timestep_assembly():
    "[steps, batch]: column b = the timesteps of the slot sample b follows; switching or re-targeting rewrites the columns concerned"
    loop = stub_loop(batch=4, steps=5)
    base = torch.arange(5, dtype=torch.float32)
    assert loop._assemble_times([1, 0, 0, 1]).shape == (5, 4)
    loop(torch.ones(4, 2), slot=[1, 0, 0, 1])
    assert loop.sample_times.shape == (5, 4)
    for b, k in enumerate([1, 0, 0, 1]):
        assert torch.equal(loop.sample_times[:, b], base + 100.0 * k)
    assert torch.equal(loop.static_times, base)  # what wrapper.step looks its index up in is the wrapper's own: untouched
    loop(torch.ones(4, 2), slot=1)
    assert torch.equal(loop.sample_times, (base + 100.0).unsqueeze(1).repeat(1, 4))
    loop(torch.ones(4, 2), slot=[0, 0, 1, 0])
    assert torch.equal(loop.sample_times[:, 2], base + 100.0) and torch.equal(loop.sample_times[:, 0], base)


def test_retarget_rewrites_the_columns_that_follow_the_slot():
    class Rows(StubRows):
        cursor = 0

        def begin(self, mode, slot=0):
            self.cursor = self.length

        def upload(self, slot):
            pass

    class Wrapper:
        timesteps = torch.arange(5, dtype=torch.float32) + 500.0

    loop = stub_loop(batch=4, steps=5)
    loop.rows.__class__ = Rows
    shapes = []
    loop._runner = lambda wrapper, x: shapes.append(tuple(x.shape))
    loop(torch.ones(4, 2), slot=[1, 0, 0, 1])
    loop.retarget(Wrapper(), slot=2)  # nobody follows slot 2: no column changes
    assert shapes == [(1, 2)] and 2 in loop._filled  # (the dry run is on one sample)
    assert torch.equal(loop.sample_times[:, 1], torch.arange(5.0)) and torch.equal(loop.sample_times[:, 0], torch.arange(5.0) + 100.0)
    loop.retarget(Wrapper(), slot=1)  # samples 0 and 3 follow slot 1
    assert torch.equal(loop.sample_times[:, 1], torch.arange(5.0))
    assert torch.equal(loop.sample_times[:, 0], Wrapper.timesteps) and torch.equal(loop.sample_times[:, 3], Wrapper.timesteps)


def test_export_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"^int " + NAME + r"\(", header, flags=re.M)
    assert "const int32_t* sample_index_dev" in header and "nor clamps" in header  # index validity is documented as the caller's
    assert NAME in _hip.EXPORTS
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, NAME)
    lib.skr_abi_version.restype = ctypes.c_int
    assert lib.skr_abi_version() == _hip.ABI_VERSION == 15 == int(re.search(r"#define SKR_ABI_VERSION (\d+)", header).group(1))


def test_argument_validation_without_gpu():
    lib = _hip.load()
    plan = _hip.StepPlanC()
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), None, None, None, None, 4096, None, None, 0, None) == 1  # SKR_ERR_NULL: no rows
    rows = (_hip.StepRowC * 1)()
    index = (ctypes.c_int32 * 2)()
    assert lib.skr_step_launch_indexed_per_sample(ctypes.byref(plan), None, None, None, None, 4096, ctypes.addressof(rows), None, 0, None) == 1  # no index
    assert lib.skr_step_launch_indexed_per_sample(None, None, None, None, None, 4096, ctypes.addressof(rows), ctypes.addressof(index), 0, None) == 1


def test_header_with_the_new_entry_is_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "h.c"
    src.write_text(f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
                   "typedef int (*entry)(const skr_step_plan*, const void* const*, void*, void*, const uint64_t*, int64_t, const skr_step_row*, const int32_t*, int32_t, void*);\n"
                   f"int main(void) {{ entry e = {NAME}; return e ? 0 : 1; }}\n")  # fmt: skip
    assert subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "h.o")], capture_output=True).returncode == 0
