"""Device-resident positions of rolling batches without a GPU: the `skr_rolling_advance` export and its argument checks, and the
bookkeeping of `RollingBatch(device_positions=True)` on stubs (the dry run, the step launch and the advance launch are replaced;
the advance runs `rolling.advance_reference` on CPU tensors: nothing here enqueues device work)."""

import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
from conftest import ROOT

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.rolling import RollingBatch, advance_reference
from skrample_amd.sampling import structured as PT

NAME = "skr_rolling_advance"
WIDE = [("x",), ("o",), ("pi", -1), ("po", -1), ("pi", -2), ("po", -2)]
SENTINEL = -77


def test_export_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"^int " + NAME + r"\(", header, flags=re.M)
    assert "0 <= p < n <= max_steps" in header and "keep their bytes" in header
    assert NAME in _hip.EXPORTS
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, NAME)
    lib.skr_abi_version.restype = ctypes.c_int
    assert lib.skr_abi_version() == _hip.ABI_VERSION == 15 == int(re.search(r"#define SKR_ABI_VERSION (\d+)", header).group(1))  # purely additive


def test_header_with_the_new_entry_is_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    src = tmp_path / "h.c"
    src.write_text(f'#include "{os.path.join(ROOT, "include", "skrample_hip.h")}"\n'
                   "typedef int (*entry)(int32_t*, const int32_t*, const float*, int32_t*, float*, int32_t, int32_t, void*);\n"
                   f"int main(void) {{ entry e = {NAME}; return e ? 0 : 1; }}\n")  # fmt: skip
    assert subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "h.o")], capture_output=True).returncode == 0


def test_argument_validation_without_gpu():
    "host buffers stand in for device pointers: every check precedes the launch and none dereferences"
    lib = _hip.load()
    ints = [(ctypes.c_int32 * 4)() for _ in range(3)]
    floats = [(ctypes.c_float * 4)() for _ in range(2)]
    good = [ctypes.addressof(ints[0]), ctypes.addressof(ints[1]), ctypes.addressof(floats[0]), ctypes.addressof(ints[2]), ctypes.addressof(floats[1])]
    for k in range(5):
        args = list(good)
        args[k] = None
        assert lib.skr_rolling_advance(*args, 4, 1, None) == 1, k  # SKR_ERR_NULL
    assert lib.skr_rolling_advance(*good, 0, 1, None) == 5  # SKR_ERR_SHAPE
    assert lib.skr_rolling_advance(*good, 4, 0, None) == 5
    assert lib.skr_rolling_advance(*good, -1, 1, None) == 5
    assert lib.skr_rolling_advance(*good, 65536, 65536, None) == 5  # capacity * max_steps past INT32_MAX
    assert lib.skr_rolling_advance(None, None, None, None, None, 0, 0, None) == 1


def test_advance_reference():
    times = [float(i) for i in range(12)]
    position, index, timestep = advance_reference([0, 2, 3, -1], [3, 3, 3, 2], times, 3)
    assert position == [1, 3, 3, -1] and index == [0, 5, -1, -1] and timestep == [0.0, 5.0, None, None]
    assert advance_reference([0, 0], [0, 4], times, 3) == ([0, 0], [-1, -1], [None, None])  # free; a run longer than max_steps


# ---- RollingBatch on stubs ------------------------------------------------------------------------------------------------


def stub_plan(n_terms: int, scale: float = 1.0) -> _hip.StepPlanC:
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n_terms
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.NONE
    for k in range(n_terms):
        plan.coef0[k] = scale * (k + 1)
    return plan


class StubBatch(RollingBatch):
    "the dry run gives a DPM-3-like ramp-up; step launches are counted, not made; the advance is `advance_reference` on the CPU tables"

    launches = 0
    traces = 0
    advances = 0

    def _trace(self, wrapper, steps, seed):
        self.traces += 1
        return [(stub_plan(min(2 * (i + 1), 6), scale=10.0 * (i + 1)), WIDE[: min(2 * (i + 1), 6)], 100.0 - i) for i in range(steps)]

    def _launch(self, arr, out0, out1):
        self.launches += 1

    def _advance(self):
        self.advances += 1
        position, index, timestep = advance_reference(self.position_dev.tolist(), self.length_dev.tolist(), self.times_dev.tolist(), self.max_steps)
        self.position_dev.copy_(torch.tensor(position, dtype=torch.int32))
        self.index_dev.copy_(torch.tensor(index, dtype=torch.int32))
        for b, t in enumerate(timestep):
            if t is not None:
                self.timesteps[b] = t


def wrapper(order=3, eta=0.0):
    return PD.SkrampleWrapperScheduler(PT.DPM(order=order, stochasticity=eta), PS.Scaled())


def stub_batch(capacity=4, **options):
    return StubBatch(wrapper, torch.zeros(capacity, 4, 32, 32, dtype=torch.bfloat16), capacity=capacity, **options)


def scenario(batch, tick):
    """`test_index_vectors_for_staggered_positions` of test_rolling_host.py: admissions at different ticks, two slots that finish on
    the same tick, a slot reused after take().  `tick(batch, out)` makes one tick with its own checks and returns (the finished
    slots, the index the tick used)."""
    x = torch.ones(4, 32, 32, dtype=torch.bfloat16)
    out = torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16)
    seen = []
    batch.admit(1, x, wrapper(), 3)
    seen.append(tick(batch, out.clone()))
    assert seen[-1][0] == []
    batch.admit(3, x * 2, wrapper(), 2)
    seen.append(tick(batch, out.clone()))
    assert seen[-1][0] == []
    seen.append(tick(batch, out.clone()))
    assert sorted(seen[-1][0]) == [1, 3] and batch.active == [] and batch.index_vector() == [-1] * 4
    batch.take(3)
    batch.admit(3, x, wrapper(), 4)  # free again at once, while slot 1 still holds its result
    seen.append(tick(batch, out.clone()))
    assert batch.take(1).shape == (4, 32, 32)
    return seen


# what the host path publishes: the index of every tick, and the timesteps the network of that tick reads
INDEX = [[-1, 16, -1, -1], [-1, 17, -1, 48], [-1, 18, -1, 49], [-1, -1, -1, 48]]
TIMES = [[0.0, 100.0, 0.0, 0.0], [0.0, 99.0, 0.0, 100.0], [0.0, 98.0, 0.0, 99.0], [0.0, 98.0, 0.0, 100.0]]


def test_host_published_ticks_are_untouched():
    "device_positions=False: step() publishes the index as before, and there is nothing to advance"
    batch = stub_batch(capacity=4, max_steps=16)
    assert not batch.device_positions and not hasattr(batch, "position_dev")
    at = []

    def tick(batch, out):
        expect, times = batch.index_vector(), batch.timesteps.tolist()  # (the host path publishes timesteps ahead of the tick)
        with pytest.raises(ValueError, match="needs device_positions=True"):
            batch.advance()
        done = batch.step(out)
        assert batch.index_dev.tolist() == expect  # published by step()
        at.append((expect, times))
        return done, expect

    scenario(batch, tick)
    assert [i for i, _ in at] == INDEX and [t for _, t in at] == TIMES  # the constants below describe today's host path
    assert batch.launches == 4 and batch.advances == 0
    with pytest.raises(ValueError, match="needs device_positions=True"):
        batch.capture(lambda x, t: x)


def test_device_positions_bookkeeping_on_stubs():
    batch = stub_batch(capacity=4, max_steps=16, device_positions=True)
    assert batch.position_dev.dtype == batch.length_dev.dtype == torch.int32 and batch.times_dev.dtype == torch.float32
    assert batch.position_dev.shape == batch.length_dev.shape == (4,) and batch.times_dev.shape == (64,)
    n = [0]

    def tick(batch, out):
        launches = batch.launches
        with pytest.raises(ValueError, match="advance"):  # step() without advance(): refused before any launch
            batch.step(out)
        assert batch.launches == launches and batch.index_dev.tolist() != batch.index_vector()
        expect = batch.index_vector()
        batch.advance()
        assert batch.index_dev.tolist() == expect == INDEX[n[0]]  # the device's index is the host mirror's
        assert batch.timesteps.tolist() == TIMES[n[0]]  # ... and its timesteps what the host path publishes for this tick
        with pytest.raises(ValueError, match="already"):
            batch.advance()
        with pytest.raises(ValueError, match="between advance"):  # this tick's index is on the device: admissions wait for step()
            batch.admit(0, torch.ones(4, 32, 32, dtype=torch.bfloat16), wrapper(), 3)
        batch.index_dev.fill_(SENTINEL)  # sealed: step() must not publish anything from the host
        held_times = batch.timesteps.clone()
        done = batch.step(out)
        assert batch.index_dev.tolist() == [SENTINEL] * 4 and torch.equal(batch.timesteps, held_times)
        assert batch.launches == launches + 1
        n[0] += 1
        return done, expect

    scenario(batch, tick)
    assert batch.launches == 4 and batch.advances == 4
    # the tables after the scenario: slot 1 was taken (length 0), slot 3 is at position 1 of 4
    assert batch.length_dev.tolist() == [0, 0, 0, 4] and batch.position_dev.tolist()[3] == 1
    assert batch.times_dev[48:52].tolist() == [100.0, 99.0, 98.0, 97.0]
    batch._requests[3].position = 7  # a mirror position outside the run is refused before any launch
    with pytest.raises(ValueError, match="position 7 of a run of 4"):
        batch.advance()
    assert batch.advances == 4 and batch.launches == 4


def test_every_refusal_comes_before_any_launch_or_table_write():
    batch = stub_batch(device_positions=True)
    x = torch.ones(4, 32, 32, dtype=torch.bfloat16)
    out = torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16)
    tables = lambda: [t.clone() for t in (batch.position_dev, batch.length_dev, batch.times_dev, batch.index_dev, batch.timesteps, batch.rows_dev)]  # noqa: E731
    before, traces = tables(), batch.traces
    with pytest.raises(ValueError, match="no active slot"):
        batch.step(out)
    with pytest.raises(ValueError, match="no active slot"):
        batch.advance()
    for slot in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="outside 0..3"):
            batch.admit(slot, x, wrapper(), 3)
    with pytest.raises(ValueError, match="outside 0..3"):
        batch.take(9)
    with pytest.raises(ValueError, match="sampler structure"):
        batch.admit(0, x, wrapper(order=2), 3)
    with pytest.raises(ValueError, match="draws noise"):
        batch.admit(0, x, wrapper(eta=1.0), 3, seed=1)
    with pytest.raises(ValueError, match="1..128 steps"):
        batch.admit(0, x, wrapper(), 129)
    with pytest.raises(ValueError, match="latents of shape"):
        batch.admit(0, x[:2], wrapper(), 3)
    with pytest.raises(ValueError, match="holds no request"):
        batch.take(0)
    assert batch.traces == traces and batch.launches == 0 and batch.advances == 0
    assert all(torch.equal(a, b) for a, b in zip(before, tables()))
    batch.admit(0, x, wrapper(), 3)
    assert batch.length_dev.tolist() == [3, 0, 0, 0] and batch.position_dev.tolist() == [0] * 4 and batch.times_dev[:4].tolist() == [100.0, 99.0, 98.0, 0.0]
    before = tables()
    with pytest.raises(ValueError, match="slot 0 is busy"):
        batch.admit(0, x, wrapper(), 3)
    with pytest.raises(ValueError, match="has not finished: 0 of 3"):
        batch.take(0)
    batch.advance()
    after_advance = tables()
    with pytest.raises(ValueError, match="model output of a tick"):
        batch.step(out[:2])
    assert batch.launches == 0 and all(torch.equal(a, b) for a, b in zip(after_advance, tables()))
    assert torch.equal(before[5], after_advance[5])  # (an advance leaves the rows alone)
    with pytest.raises(ValueError, match="resident request"):  # capture() refuses before any device work
        batch.capture(lambda x, t: x)
    assert batch.step(out) == [] and batch.launches == 1
    with pytest.raises(ValueError, match="int32"):
        StubBatch(wrapper, torch.zeros(1, 4, 32, 32, dtype=torch.bfloat16), capacity=65536, max_steps=65536, device_positions=True)
