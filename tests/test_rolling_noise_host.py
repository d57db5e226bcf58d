"""Structured noise in rolling batches without a GPU: the two exports at the C boundary and their argument checks, and the bookkeeping
of a structured-noise `skrample_amd.rolling.RollingBatch` on stub rows (the dry run, the draw, the launch and the advance are replaced:
nothing here enqueues device work)."""

import ctypes
import os
import re

import pytest
import torch
from conftest import ROOT

import skrample_amd.diffusers as PD
import skrample_amd.scheduling as PS
from skrample_amd import _hip
from skrample_amd.pytorch import noise as N
from skrample_amd.rolling import CapturedTicks, RollingBatch, draw_reference, place_row
from skrample_amd.sampling import structured as PT

NAMES = ("skr_noise_offset_rolling", "skr_noise_pyramid_rolling")
UNIT = (4, 32, 32)
# a UniPC-like structure: the corrector re-evaluates the previous step with the previous draw
WIDE = [("x",), ("o",), ("n",), ("pi", -1), ("po", -1), ("pn", -1)]


def test_exports_are_declared_listed_and_built():
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert re.search(r"^int " + name + r"\(", header, flags=re.M) and name in _hip.EXPORTS and hasattr(lib, name)
    assert "sample_index_dev[b] - b * rows_per_slot" in header and "inactive" in header
    lib.skr_abi_version.restype = ctypes.c_int
    assert lib.skr_abi_version() == _hip.ABI_VERSION == 15 == int(re.search(r"#define SKR_ABI_VERSION (\d+)", header).group(1))  # purely additive


def test_argument_validation_without_gpu():
    "every check precedes the launch and dereferences nothing: host buffers stand in for device memory"
    lib = _hip.load()
    buf = (ctypes.c_char * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    flat = (ctypes.c_int64 * 2)(4, 1024)
    f64 = _hip.DTYPE_CODE[torch.float64]

    def offset(out=base, dtype=_hip.BF16, seeds=base, index=base, rows=8, stride=256, batch=5, shape=flat, nd=2):
        return lib.skr_noise_offset_rolling(out, dtype, seeds, index, rows, stride, 0, batch, shape, nd, 1, 0.2, None)

    def pyramid(out=base, dtype=_hip.BF16, scratch=base, partials=base, levels=base, seeds=base, index=base, rows=8, stride=256, batch=5, unit=UNIT, resize_h=1, depth=99):
        return lib.skr_noise_pyramid_rolling(out, dtype, scratch, partials, levels, seeds, index, rows, stride, 0, batch, *unit, resize_h, 0.3, depth, None)

    for call in (offset, pyramid):
        assert call(index=None) == 1 and call(out=None) == 1 and call(seeds=None) == 1  # SKR_ERR_NULL
        assert call(rows=0) == 5 and call(rows=-1) == 5 and call(stride=0) == 5 and call(batch=-1) == 5  # SKR_ERR_SHAPE
        assert call(rows=0x7FFFFFFF) == 5 and call(batch=65536, rows=65536) == 5  # batch * rows_per_slot past INT32_MAX
        assert call(dtype=f64) == 7 and call(dtype=17) == 2  # SKR_ERR_UNSUPPORTED: no fp64 latents in a rolling batch; SKR_ERR_DTYPE
        assert call(batch=0) == 0 and call(batch=0, out=None, index=None) == 0  # an empty batch: SKR_OK, nothing launched
        assert call(batch=0, rows=0) == 5  # (the draw arguments are checked first)
    assert pyramid(scratch=None) == 1 and pyramid(partials=None) == 1 and pyramid(levels=None) == 1
    assert pyramid(unit=(3, 30, 90)) == 7 and pyramid(unit=(1, 512, 512)) == 7 and pyramid(unit=(4, 32, 30)) == 7  # outside the LDS route / w % 4
    assert pyramid(unit=(4, 2, 32), resize_h=0) == 5 and pyramid(depth=-1) == 5 and pyramid(unit=(0, 32, 32)) == 5  # as skr_noise_pyramid
    assert pyramid(batch=65536, rows=1) == 7 and offset(batch=65536, rows=1) == 7  # gridDim.y
    assert offset(shape=(ctypes.c_int64 * 2)(512, 4)) == 7 and offset(out=base + 8) == 7  # innermost axis 4; `out` not 16-byte aligned
    assert offset(nd=5) == 5 and offset(shape=None) == 5 and offset(shape=(ctypes.c_int64 * 2)(0, 1024)) == 0  # as skr_noise_offset (an empty unit: SKR_OK)
    # the probes answer what the entries would, with nothing launched
    assert lib.skr_noise_pyramid_rolling_covers(8, *UNIT, 1) == 0 and lib.skr_noise_pyramid_rolling_covers(8, 1, 512, 512, 1) == 7
    assert lib.skr_noise_offset_rolling_covers(8, flat, 2) == 0 and lib.skr_noise_offset_rolling_covers(8, (ctypes.c_int64 * 2)(512, 4), 2) == 7


def test_draw_numbers_against_a_plain_restatement():
    "slot b at row index[b] of a table of max_steps rows per slot: draw d = its position, streams d * 256 (+1, or the first draw's when static)"
    index, max_steps = [-1, 16 + 3, -1, 48, 64 + 15], 16
    restated = []
    for b, at in enumerate(index):
        position = at - b * max_steps
        restated.append(None if at < 0 else (position * N.SUBSTREAMS, position * N.SUBSTREAMS))
    assert draw_reference(index, max_steps, static=False) == restated == [None, (768, 768), None, (0, 0), (3840, 3840)]
    assert draw_reference(index, max_steps, static=True) == [None, (768, 0), None, (0, 0), (3840, 0)]
    # what a lone generator counts: draw n of it owns the streams n * SUBSTREAMS .. (the first draw's for a static generator's auxiliary stream)
    lone = N.Offset.from_inputs(UNIT, 5, N.OffsetProps(), torch.bfloat16)
    assert [lone._next_stream() for _ in range(4)] == [d * N.SUBSTREAMS for d in range(4)]


# ---- RollingBatch on stub rows ------------------------------------------------------------------------------------------------
def stub_plan(n_terms: int, scale: float, two: bool) -> _hip.StepPlanC:
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = n_terms
    plan.dtype_a = plan.dtype_b = plan.out0_dtype = _hip.BF16
    plan.out1_dtype = _hip.BF16 if two else _hip.NONE
    for k in range(n_terms):
        plan.coef0[k] = scale * (k + 1)
    return plan


class StubBatch(RollingBatch):
    """the dry run of a drawing wrapper gives (x, o, n) for the first step and the wide structure afterwards -- the last step's noise
    coefficient is zero -- and (x, o) / (x, o, pi, po) for one that does not draw; draws, launches and advances are logged, not made"""

    wide = WIDE

    def __init__(self, *args, **kwargs):
        self.log, self.traces = [], 0
        super().__init__(*args, **kwargs)

    def _trace(self, wrapper, steps, seed):
        self.traces += 1
        draws = bool(wrapper.sampler.require_noise)
        found = []
        for i in range(steps):
            roles = [r for r in (self.wide[:3] if i == 0 else self.wide) if draws or r[0] not in ("n", "pn")]
            plan = stub_plan(len(roles), 10.0 * (i + 1), two=False)
            if draws and i == steps - 1:
                plan.coef0[roles.index(("n",))] = 0.0
            found.append((plan, roles, 100.0 - i))
        return found

    def _draw(self, out):
        self.log.append(("draw", out.data_ptr(), self.index_dev.tolist()))

    def _launch(self, arr, out0, out1):
        self.log.append(("launch", list(arr), self.index_dev.tolist()))

    def _advance(self):
        self.log.append(("advance",))
        self.index_dev.copy_(torch.tensor(self.index_vector(), dtype=torch.int32))  # (what the kernel would publish)


def wrapper(noise_type=N.Pyramid, props=None, eta=1.0, **options):
    return PD.SkrampleWrapperScheduler(PT.UniPC(order=2, stochasticity=eta), PS.Scaled(), noise_type=noise_type, noise_props=props, **options)


def stub_batch(capacity=4, make=wrapper, **options):
    return StubBatch(make, torch.zeros(capacity, *UNIT, dtype=torch.bfloat16), capacity=capacity, **options)


def test_noise_roles_get_slots_and_the_plan_draws_nothing_itself():
    batch = stub_batch()
    assert batch.structured and batch.draws_noise and batch.roles == WIDE and batch.plan.noise_mode == 0
    assert batch.noise_type is N.Pyramid and batch.noise_props == N.PyramidProps()
    assert len(batch._n) == len(batch._x) == batch.keep + 2 and all(tuple(t.shape) == (4, *UNIT) and t.dtype == torch.bfloat16 for t in batch._n)
    scratch, levels, partials = batch._noise_ws  # for `capacity` samples, allocated once
    assert (scratch.numel(), scratch.dtype, levels.numel(), partials.numel(), partials.dtype) == (4 * 4096, torch.float32, 4 * 17, 4 * 4 * 2, torch.float64)
    narrow = stub_plan(3, 2.0, two=False)
    row = place_row(WIDE, narrow, [("x",), ("n",), ("pn", -1)], two_outputs=False)
    assert list(row.coef0)[:6] == [2.0, 0.0, 4.0, 0.0, 0.0, 6.0] and (row.zeta0, row.stream0, row.zeta1, row.stream1) == (0.0, 0, 0.0, 0)
    batch.admit(1, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(), 4, seed=(1 << 64) - 2)
    rows = batch._requests[1].rows
    at_n, at_pn = WIDE.index(("n",)), WIDE.index(("pn", -1))
    assert [r.coef0[at_n] for r in rows] == [30.0, 60.0, 90.0, 0.0]  # the noise operand's coefficient travels like any operand's; the last step's is zero
    assert [r.coef0[at_pn] for r in rows] == [0.0, 120.0, 180.0, 240.0]  # a first row never reads the slot's previous occupant's draw
    assert all(r.zeta0 == r.zeta1 == 0.0 and r.stream0 == r.stream1 == 0 for r in rows) and batch.seeds_dev.tolist()[1] == -2
    # a sampler whose steps read no earlier draw: one noise tensor, no ring (and Offset keeps no workspace)
    class NoEarlierDraw(StubBatch):
        wide = WIDE[:5]

    single = NoEarlierDraw(lambda: wrapper(N.Offset), torch.zeros(4, *UNIT, dtype=torch.bfloat16), capacity=4)
    assert single.noise_type is N.Offset and single._noise_ws == () and single.roles == WIDE[:5] and len(single._n) == 1 and len(single._x) == single.keep + 2
    # a Random batch is what it was: noise_mode 1, no noise tensors, no generator
    plain = stub_batch(make=lambda: wrapper(N.Random))
    assert not plain.structured and plain.plan.noise_mode == 1 and not hasattr(plain, "_n") and not hasattr(plain, "noise_type")
    quiet = stub_batch(make=lambda: wrapper(N.Colored, eta=0.0))  # a sampler that does not draw: the generator class does not matter
    assert not quiet.structured and not quiet.draws_noise and quiet.plan.noise_mode == 0


def test_the_step_launch_of_a_structured_batch_gets_no_seeds(monkeypatch):
    calls = []

    class Lib:
        def skr_step_launch_rolling(self, *args):
            calls.append(args)
            return 0

    structured, plain = stub_batch(), stub_batch(make=lambda: wrapper(N.Random))
    monkeypatch.setattr(_hip, "load", lambda: Lib())
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: 0)
    out = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    arr = (ctypes.c_void_p * 1)(out.data_ptr())
    RollingBatch._launch(structured, arr, out, None)
    RollingBatch._launch(plain, arr, out, None)
    assert len(calls) == 2 and all(len(c) == 10 for c in calls)
    assert calls[0][4] is None and calls[1][4] == plain.seeds_dev.data_ptr()


def test_the_draw_call_of_each_generator(monkeypatch):
    "one call of the generator's rolling entry: the batch's tensors, the index vector, max_steps rows per slot, 256 streams per draw, the props"
    calls = []

    class Lib:
        def skr_noise_offset_rolling(self, *args):
            calls.append(("offset", args))
            return 0

        def skr_noise_pyramid_rolling(self, *args):
            calls.append(("pyramid", args))
            return 0

    pyramid = stub_batch(make=lambda: wrapper(N.Pyramid, N.PyramidProps(strength=0.5, depth=3, static=True)), max_steps=16)
    offset = stub_batch(make=lambda: wrapper(N.Offset, N.OffsetProps(dims=(0, 2), strength=0.25)), max_steps=16)
    monkeypatch.setattr(_hip, "load", lambda: Lib())
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: 0)
    RollingBatch._draw(pyramid, pyramid._n[-1])
    RollingBatch._draw(offset, offset._n[-1])
    (_, p), (_, o) = calls
    scratch, levels, partials = pyramid._noise_ws
    assert p[:7] == (pyramid._n[-1].data_ptr(), _hip.BF16, scratch.data_ptr(), partials.data_ptr(), levels.data_ptr(), pyramid.seeds_dev.data_ptr(), pyramid.index_dev.data_ptr())
    assert p[7:] == (16, 256, 1, 4, 4, 32, 32, 1, 0.5, 3, 0)
    assert o[:4] == (offset._n[-1].data_ptr(), _hip.BF16, offset.seeds_dev.data_ptr(), offset.index_dev.data_ptr()) and o[4:8] == (16, 256, 0, 4)
    assert list(o[8]) == [4, 32, 32] and o[9:] == (3, 0b101, 0.25, 0)


def test_the_draw_precedes_the_launch_and_the_noise_ring_rotates():
    batch = stub_batch(max_steps=16)
    x = torch.zeros(UNIT, dtype=torch.bfloat16)
    batch.admit(2, x, wrapper(), 8, seed=3)
    ring, P = [t.data_ptr() for t in batch._n], len(batch._x)  # oldest first; as long as the latents ring
    at_n, at_pn = WIDE.index(("n",)), WIDE.index(("pn", -1))
    for tick in range(P + 1):
        batch.step(torch.zeros(4, *UNIT, dtype=torch.bfloat16))
        (draw, target, seen_by_draw), (launch, ptrs, seen_by_launch) = batch.log[-2:]
        assert (draw, launch) == ("draw", "launch") and seen_by_draw == seen_by_launch == [-1, -1, 32 + tick, -1]  # the index is on the device before both
        assert target == ring[tick % P] == ptrs[at_n] == batch._n[-1].data_ptr()  # the oldest draw's tensor takes this tick's
        assert ptrs[at_pn] == ring[(tick - 1) % P]  # ... and the previous tick's draw is one place behind
        if tick == P - 1:
            assert [t.data_ptr() for t in batch._n] == ring  # P ticks bring the ring back
    assert [t.data_ptr() for t in batch._n] == ring[1:] + ring[:1] and len(batch.log) == 2 * (P + 1)


def test_device_positions_draw_after_the_advance():
    batch = stub_batch(max_steps=16, device_positions=True)
    batch.admit(0, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(), 3, seed=3)
    batch.advance()
    batch.step(torch.zeros(4, *UNIT, dtype=torch.bfloat16))
    assert [entry[0] for entry in batch.log] == ["advance", "draw", "launch"] and batch.log[1][2] == [0, -1, -1, -1]


def test_captured_ticks_bind_the_noise_ring_per_phase_and_draw_between_replay_and_launch():
    "CapturedTicks without its graphs: the per-phase binding and the order of a tick (replay, draw, launch)"
    batch = stub_batch(max_steps=16, device_positions=True)
    batch.admit(3, torch.zeros(UNIT, dtype=torch.bfloat16), wrapper(), 8, seed=3)

    class Graph:
        def __init__(self, p):
            self.p = p

        def replay(self):
            batch.log.append(("replay", self.p))
            batch._advance()

    ticks = object.__new__(CapturedTicks)
    ticks.batch, ticks.phases, ticks.ticks, ticks.replays = batch, len(batch._x), 0, [0] * len(batch._x)
    ticks.outputs = [torch.zeros(4, *UNIT, dtype=torch.bfloat16) for _ in range(ticks.phases)]
    ticks.graphs = [Graph(p) for p in range(ticks.phases)]
    ring, P = [t.data_ptr() for t in batch._n], ticks.phases
    ticks._bind_phases()
    at_n, at_pn = WIDE.index(("n",)), WIDE.index(("pn", -1))
    assert [t.data_ptr() for t in ticks._draws] == ring
    for p, (arr, *_) in enumerate(ticks._launches):
        assert arr[at_n] == ring[p] and arr[at_pn] == ring[(p - 1) % P]
    for tick in range(P + 1):  # past one period
        ticks.tick()
        assert [entry[0] for entry in batch.log[-4:]] == ["replay", "advance", "draw", "launch"]
        assert batch.log[-2][1] == ring[tick % P] == batch.log[-1][1][at_n] and batch.log[-1][1][at_pn] == ring[(tick - 1) % P]
        assert batch.log[-2][2] == [-1, -1, -1, 48 + tick] and batch._n[-1].data_ptr() == ring[tick % P]  # the batch's ring follows


def test_refusals_when_the_batch_is_built_and_at_admit():
    class Custom(N.Pyramid):
        pass

    example = torch.zeros(4, *UNIT, dtype=torch.bfloat16)
    for noise_type, match in ((N.Colored, "Colored noise cannot join"), (N.Brownian, "Brownian noise cannot join"), (Custom, "custom generator class")):
        with pytest.raises(_hip.SkrampleHipError, match=match):
            stub_batch(make=lambda: wrapper(noise_type))
    with pytest.raises(ValueError, match="prefetch_noise=True"):
        stub_batch(make=lambda: wrapper(prefetch_noise=True))
    with pytest.raises(ValueError, match="inpaint_mask_shape together with Offset noise"):
        StubBatch(lambda: wrapper(N.Offset), example, capacity=4, inpaint_mask_shape=(1, 32, 32))
    with pytest.raises(_hip.SkrampleHipError, match="outside the LDS route"):
        StubBatch(wrapper, torch.zeros(2, 1, 512, 512, dtype=torch.bfloat16), capacity=2)
    with pytest.raises(_hip.SkrampleHipError, match="no rolling form"):
        stub_batch(make=lambda: wrapper(props=N.PyramidProps(dims=(0, 2))))
    with pytest.raises(_hip.SkrampleHipError, match="outside the aligned Offset kernel"):
        StubBatch(lambda: wrapper(N.Offset, N.OffsetProps(dims=(0, 2))), torch.zeros(2, 4, 128, 4, dtype=torch.bfloat16), capacity=2)
    batch = stub_batch()
    x, traces = torch.zeros(UNIT, dtype=torch.bfloat16), batch.traces
    with pytest.raises(ValueError, match="noise_props"):
        batch.admit(0, x, wrapper(props=N.PyramidProps(depth=2)), 3, seed=1)
    with pytest.raises(ValueError, match="sampler structure"):
        batch.admit(0, x, wrapper(N.Offset), 3, seed=1)
    with pytest.raises(ValueError, match="needs a seed"):
        batch.admit(0, x, wrapper(), 3)
    assert batch.traces == traces and batch.free(0) and not batch.rows_dev.any()
    batch.admit(0, x, wrapper(props=N.PyramidProps()), 3, seed=1)  # the defaults, spelled out
    batch.admit(1, x, wrapper(eta=0.0), 3)  # a request that does not draw shares the batch: rows without the noise roles
    assert all(r.coef0[WIDE.index(("n",))] == 0.0 and r.coef0[WIDE.index(("pn", -1))] == 0.0 for r in batch._requests[1].rows)
