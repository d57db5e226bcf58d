"""Rolling batches without a GPU: the new export at the C boundary, its argument checks, and the bookkeeping of
`skrample_amd.rolling.RollingBatch` on stub rows (the dry run and the launch are replaced: nothing here enqueues device work)."""

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
from skrample_amd.rolling import RollingBatch, place_row
from skrample_amd.sampling import structured as PT

NAME = "skr_step_launch_rolling"
WIDE = [("x",), ("o",), ("pi", -1), ("po", -1), ("pi", -2), ("po", -2)]


def test_export_is_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    assert re.search(r"^int " + NAME + r"\(", header, flags=re.M)
    assert "inactive sample" in header and "absent operand" in header and "operand order" in header
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
                   "typedef int (*entry)(const skr_step_plan*, const void* const*, void*, void*, const uint64_t*, int64_t, const skr_step_row*, const int32_t*, int32_t, void*);\n"
                   f"int main(void) {{ entry e = {NAME}; return e ? 0 : 1; }}\n")  # fmt: skip
    assert subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c", str(src), "-o", str(tmp_path / "h.o")], capture_output=True).returncode == 0


def test_argument_validation_without_gpu():
    "the error codes of skr_step_launch_indexed_per_sample for the same bad arguments (every check precedes the launch)"
    lib = _hip.load()
    plan = _hip.StepPlanC()
    rows = (_hip.StepRowC * 1)()
    index = (ctypes.c_int32 * 2)()
    assert lib.skr_step_launch_rolling(ctypes.byref(plan), None, None, None, None, 4096, None, ctypes.addressof(index), 0, None) == 1  # SKR_ERR_NULL: no rows
    assert lib.skr_step_launch_rolling(ctypes.byref(plan), None, None, None, None, 4096, ctypes.addressof(rows), None, 0, None) == 1  # no index
    assert lib.skr_step_launch_rolling(None, None, None, None, None, 4096, ctypes.addressof(rows), ctypes.addressof(index), 0, None) == 1  # no plan
    # a well-formed request up to the sample size: host buffers stand in (16-byte aligned; no check dereferences them)
    buf = (ctypes.c_char * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    ptrs = (ctypes.c_void_p * 1)(base)
    seeds = (ctypes.c_uint64 * 2)()
    plan.n_terms, plan.n_group_a, plan.dtype_a, plan.dtype_b, plan.out0_dtype, plan.out1_dtype = 1, 1, _hip.BF16, _hip.BF16, _hip.BF16, _hip.NONE
    args = (ctypes.addressof(rows), ctypes.addressof(index), 0, None)
    for call in (lib.skr_step_launch_rolling, lib.skr_step_launch_indexed_per_sample):
        plan.sample_numel, plan.noise_mode = 1024, 1  # half a chunk: a workgroup would span two samples
        assert call(ctypes.byref(plan), ptrs, base, None, ctypes.addressof(seeds), 4096, *args) == 7  # SKR_ERR_UNSUPPORTED
        plan.noise_mode = 0  # ... with or without noise
        assert call(ctypes.byref(plan), ptrs, base, None, None, 4096, *args) == 7
        plan.sample_numel = 0  # no sample size, no batch
        assert call(ctypes.byref(plan), ptrs, base, None, None, 4096, *args) == 5  # SKR_ERR_SHAPE
        plan.noise_mode = 1
        assert call(ctypes.byref(plan), ptrs, base, None, ctypes.addressof(seeds), 4096, *args) == 5


# ---- RollingBatch on stub rows ------------------------------------------------------------------------------------------


def stub_plan(n_terms: int, scale: float = 1.0, two: bool = False) -> _hip.StepPlanC:
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n_terms
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.BF16 if two else _hip.NONE
    for k in range(n_terms):
        plan.coef0[k] = scale * (k + 1)
    return plan


class StubBatch(RollingBatch):
    "the dry run gives a DPM-3-like ramp-up (2, 4, 6, 6, ... operands); launches are counted, not made"

    launches = 0
    traces = 0

    def _trace(self, wrapper, steps, seed):
        self.traces += 1
        return [(stub_plan(min(2 * (i + 1), 6), scale=10.0 * (i + 1)), WIDE[: min(2 * (i + 1), 6)], 100.0 - i) for i in range(steps)]

    def _launch(self, arr, out0, out1):
        self.launches += 1


def wrapper(order=3, eta=0.0):
    return PD.SkrampleWrapperScheduler(PT.DPM(order=order, stochasticity=eta), PS.Scaled())


def stub_batch(capacity=4, **options):
    return StubBatch(wrapper, torch.zeros(capacity, 4, 32, 32, dtype=torch.bfloat16), capacity=capacity, **options)


def test_ramp_up_rows_are_placed_by_role_with_zeros_elsewhere():
    narrow = stub_plan(3, scale=2.0)
    narrow.zeta0, narrow.stream0, narrow.chain = 0.5, 768, 0.25
    row = place_row(WIDE, narrow, [("x",), ("po", -1), ("po", -2)], two_outputs=False)
    assert list(row.coef0)[:6] == [2.0, 0.0, 0.0, 4.0, 0.0, 6.0] and not any(list(row.coef0)[6:]) and not any(row.coef1)
    assert (row.zeta0, row.stream0, row.chain) == (0.5, 768, 0.25)
    with pytest.raises(_hip.SkrampleHipError, match="no place"):
        place_row(WIDE, narrow, [("x",), ("po", -1), ("po", -3)], two_outputs=False)
    with pytest.raises(_hip.SkrampleHipError, match="differ in order"):  # present roles must keep their relative order: the sums are ordered
        place_row(WIDE, narrow, [("x",), ("po", -2), ("po", -1)], two_outputs=False)
    # a single-output first step inside a two-output structure: its result is the structure's second output
    single = place_row(WIDE, narrow, [("x",), ("o",), ("pi", -1)], two_outputs=True)
    assert list(single.coef1)[:3] == [2.0, 4.0, 6.0] and not any(single.coef0) and (single.zeta1, single.stream1, single.zeta0, single.chain) == (0.5, 768, 0.0, 0.0)
    batch = stub_batch()
    batch.admit(0, torch.zeros(4, 32, 32, dtype=torch.bfloat16), wrapper(), 5)
    rows = batch._requests[0].rows
    assert [sum(1 for c in r.coef0 if c != 0.0) for r in rows] == [2, 4, 6, 6, 6]
    assert list(rows[0].coef0)[:6] == [10.0, 20.0, 0.0, 0.0, 0.0, 0.0] and list(rows[1].coef0)[:6] == [20.0, 40.0, 60.0, 80.0, 0.0, 0.0]
    stored = bytes(batch.rows_dev[: 5 * batch.row_bytes].numpy())
    assert stored == b"".join(bytes(r) for r in rows) and not batch.rows_dev[5 * batch.row_bytes :].any()


def test_index_vectors_for_staggered_positions():
    batch = stub_batch(capacity=4, max_steps=16)
    x = torch.ones(4, 32, 32, dtype=torch.bfloat16)
    out = torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16)
    assert batch.index_vector() == [-1, -1, -1, -1]
    batch.admit(1, x, wrapper(), 3)
    assert batch.index_vector() == [-1, 16, -1, -1] and batch.timesteps.tolist()[1] == 100.0
    assert batch.step(out.clone()) == []
    batch.admit(3, x * 2, wrapper(), 2)
    assert batch.index_vector() == [-1, 17, -1, 48] and batch.index_dev.tolist() == [-1, 16, -1, -1]  # (the device copy is the last tick's)
    assert batch.timesteps.tolist() == [0.0, 99.0, 0.0, 100.0]
    assert batch.step(out.clone()) == [] and batch.index_dev.tolist() == [-1, 17, -1, 48]
    assert batch.index_vector() == [-1, 18, -1, 49]
    assert sorted(batch.step(out.clone())) == [1, 3]
    assert batch.index_vector() == [-1, -1, -1, -1] and batch.active == []  # finished slots read nothing
    assert batch.timesteps.tolist() == [0.0, 98.0, 0.0, 99.0]  # inactive slots hold the last value they had
    batch.take(3)
    batch.admit(3, x, wrapper(), 4)  # the slot is free again at once, while slot 1 still holds its result
    assert batch.index_vector() == [-1, -1, -1, 48] and batch.launches == 3
    batch.step(out.clone())
    assert batch.index_vector() == [-1, -1, -1, 49] and batch.take(1).shape == (4, 32, 32)
    batch._requests[3].position = 7  # a position outside the run never reaches the device
    with pytest.raises(ValueError, match="position 7 of a run of 4"):
        batch.step(out.clone())
    assert batch.launches == 4


def test_every_refusal_comes_before_any_launch():
    with pytest.raises(ValueError, match="per-sample rows need samples of whole 2048-element chunks, not 1024 elements"):
        StubBatch(wrapper, torch.zeros(4, 4, 16, 16, dtype=torch.bfloat16), capacity=4)
    batch = stub_batch()
    x = torch.ones(4, 32, 32, dtype=torch.bfloat16)
    out = torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16)
    traces = batch.traces
    with pytest.raises(ValueError, match="no active slot"):
        batch.step(out)
    for slot in (-1, 4, 1.0, True):
        with pytest.raises(ValueError, match="outside 0..3"):
            batch.admit(slot, x, wrapper(), 3)
    with pytest.raises(ValueError, match="outside 0..3"):
        batch.take(9)
    with pytest.raises(ValueError, match="sampler structure"):
        batch.admit(0, x, wrapper(order=2), 3)
    with pytest.raises(ValueError, match="sampler structure"):
        batch.admit(0, x, PD.SkrampleWrapperScheduler(PT.Adams(order=3), PS.Scaled()), 3)
    with pytest.raises(ValueError, match="draws noise"):
        batch.admit(0, x, wrapper(eta=1.0), 3, seed=1)
    with pytest.raises(ValueError, match="1..128 steps"):
        batch.admit(0, x, wrapper(), 129)
    with pytest.raises(ValueError, match="latents of shape"):
        batch.admit(0, x[:2], wrapper(), 3)
    with pytest.raises(ValueError, match="holds no request"):
        batch.take(0)
    assert batch.traces == traces and batch.launches == 0  # no dry run (it launches), no launch
    batch.admit(0, x, wrapper(), 3)
    with pytest.raises(ValueError, match="slot 0 is busy"):
        batch.admit(0, x, wrapper(), 3)
    with pytest.raises(ValueError, match="has not finished: 0 of 3"):
        batch.take(0)
    with pytest.raises(ValueError, match="model output of a tick"):
        batch.step(out[:2])
    assert batch.launches == 0 and batch.index_dev.tolist() == [-1] * 4  # nothing published either
    noisy = StubBatch(lambda: wrapper(eta=1.0), torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16), capacity=4)
    with pytest.raises(ValueError, match="needs a seed"):
        noisy.admit(0, x, wrapper(eta=0.5), 3)
    noisy.admit(0, x, wrapper(eta=0.0), 3)  # a request without noise in a batch that draws: rows with zeta = 0
    noisy.admit(1, x, wrapper(eta=0.5), 3, seed=(1 << 64) - 1)
    assert noisy.seeds_dev.tolist()[1] == -1


def test_history_ring_and_alias_guard():
    batch = stub_batch()
    x = torch.ones(4, 32, 32, dtype=torch.bfloat16)
    batch.admit(0, x, wrapper(), 6)
    outs = [torch.full((4, 4, 32, 32), float(i), dtype=torch.bfloat16) for i in range(4)]
    first_latents = batch.latents
    batch.step(outs[0])
    assert batch._bind(("pi", -1), outs[1]) is first_latents and batch._bind(("po", -1), outs[1]) is outs[0]
    assert batch._bind(("po", -2), outs[1]) is batch._blank  # no tick has produced it yet: only absent operands point there
    batch.step(outs[1])
    assert batch._bind(("po", -2), outs[2]) is outs[0] and batch._bind(("pi", -2), outs[2]) is first_latents
    with pytest.raises(_hip.SkrampleHipError, match="now holds this tick's model output"):
        batch.step(outs[0])  # handed back while the ring holds it
    outs[1].add_(1)
    with pytest.raises(_hip.SkrampleHipError, match="modified in place"):
        batch.step(outs[2])
    assert batch.launches == 2
    snap = stub_batch(alias_history=False)
    snap.admit(0, x, wrapper(), 6)
    static = torch.zeros(4, 4, 32, 32, dtype=torch.bfloat16)
    for i in range(4):
        snap.step(static.fill_(float(i)))  # one buffer for every tick: snapshots
    assert [float(t[0, 0, 0, 0]) for t in snap._outputs] == [2.0, 3.0] and snap.launches == 4
