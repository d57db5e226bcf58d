"""The launch table of `_hip` without a device: one rule gives every step launch's and every guidance statistic's C entry name and
argument order (`_hip.ENTRIES`), one record says what a launch is (`_hip.StepCall`), one launcher serves the five eager entry points.
The argument order against the real ABI is tests/test_launch_table_gpu.py; here the table is held to the header, to `EXPORTS`, and to the
calls the five launchers made before there was a table -- written out below as literals."""

import ctypes
import os
import re

import pytest
import torch

from skrample_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = sorted(_hip.ENTRIES)
STREAM = 77


def header_parameters(name):
    "the parameter list of `name` in include/skrample_hip.h, comments removed"
    header = open(os.path.join(ROOT, "include", "skrample_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    found = re.search(rf"^int\s+{name}\s*\((.*?)\)\s*;", flat, flags=re.M | re.S)
    assert found, name
    return [p.strip() for p in found.group(1).split(",")]


def test_the_table_has_the_22_keys():
    assert len(KEYS) == 22 and len({name for name, _ in _hip.ENTRIES.values()}) == 22
    assert [key for key in KEYS if key[0] == _hip.FACTOR] == [(_hip.FACTOR, form) for form in ("direct", "indexed", "indexed_per_sample", "rolling")]
    for kind in ("guided", "guided_rescaled", _hip.FACTOR):  # the combinations the library does not have are errors, not other routes
        with pytest.raises(_hip.SkrampleHipError, match="no channels_last form"):
            _hip.entry_name(kind, "channels_last")
        with pytest.raises(_hip.SkrampleHipError, match="no channels_last form"):
            _hip.entry_args(kind, "channels_last")


@pytest.mark.parametrize("kind,form", KEYS, ids=[f"{kind}-{form}" for kind, form in KEYS])
def test_every_key_names_an_export_and_lays_out_what_the_entry_declares(kind, form):
    name, names = _hip.ENTRIES[kind, form]
    assert name == _hip.entry_name(kind, form) and name in _hip.EXPORTS
    # the naming rule of the issue, spelled out once more
    base = "skr_guidance_rescale_factor" if kind == _hip.FACTOR else "skr_step_launch" + {"plain": ""}.get(kind, "_" + kind)
    assert name == base + ("" if form == "direct" else "_" + form)
    structures = {"plan": _hip.StepPlanC(), "mask": _hip.StepMaskC(), "guide": _hip.StepGuidanceC(), "rescale": _hip.StepRescaleC(), "layout": _hip.StepLayoutC()}
    values = {n: structures.get(n, object()) for n in _hip.ARGTYPES}  # one distinct value per name: a position can be told from any other
    args = tuple(getattr(a, "_obj", a) for a in _hip.entry_args(kind, form, **values))  # (a structure goes by reference: `_obj` is the structure)
    declared = header_parameters(name)
    assert len(args) == len(names) == len(declared), (name, names, declared)
    if os.path.isfile(_hip.LIB_PATH):
        entry = getattr(_hip.load(), name)
        assert len(entry.argtypes) == len(args) and entry.restype is ctypes.c_int
        assert entry.argtypes == [_hip.ARGTYPES[n] for n in names]
    # the positions the rule gives: (plan, operands, out0, <out1 | mask | guide | guide, rescale>, seeds, [layout,] numel, [rows, index, row_offset,] stream)
    table = form in ("indexed", "indexed_per_sample", "rolling")
    assert args[-1] is values["stream"] and re.search(r"void\s*\*\s*stream$", declared[-1])
    if table and kind != _hip.FACTOR:
        assert args[-4:-1] == (values["rows"], values["index"], values["row_offset"]) and re.search(r"int32_t\s+row_offset$", declared[-2])
    if kind == _hip.FACTOR:  # (uncond, cond, dtype, [scale,] numel, sample_numel, [rows, index, row_offset,] factor, stats, partials, stream)
        at = 3 if table else 4
        assert args[:3] == (values["uncond"], values["cond"], values["dtype"]) and (table or args[3] is values["scale"])
        assert args[at] is values["numel"] and args[at + 1] is values["sample_numel"] and re.search(r"int64_t\s+numel$", declared[at])
        assert args[-4:-1] == (values["factor"], values["stats"], values["partials"])
        if table:
            assert args[at + 2 : at + 5] == (values["rows"], values["index"], values["row_offset"]) and re.search(r"int32_t\s+row_offset$", declared[at + 4])
        return
    extras = {"plain": 1, "masked": 1, "guided": 1, "guided_rescaled": 2}[kind]
    assert args[0] is values["plan"] and args[1] is values["operands"] and args[2] is values["out0"] and re.search(r"skr_step_plan\s*\*\s*plan$", declared[0])
    assert args[3 + extras] is values["seeds"] and re.search(r"seeds_dev$", declared[3 + extras])
    numel_at = 3 + extras + 1 + (form == "channels_last")
    assert args[numel_at] is values["numel"] and re.search(r"int64_t\s+numel$", declared[numel_at])
    if form == "channels_last":
        assert args[numel_at - 1] is values["layout"] and re.search(r"skr_step_layout\s*\*\s*layout$", declared[numel_at - 1])
    assert len(args) == numel_at + 1 + (3 if table else 0) + 1


def test_every_launch_export_is_reached_from_exactly_one_key():
    launches = [n for n in _hip.EXPORTS if n.startswith(("skr_step_launch", "skr_guidance_rescale_factor"))]
    names = [name for name, _ in _hip.ENTRIES.values()]
    assert len(launches) == 22 and sorted(names) == sorted(launches) and all(names.count(n) == 1 for n in launches)


def test_structures_go_by_reference_and_unknown_names_are_ignored():
    plan, mask = _hip.StepPlanC(), _hip.StepMaskC()
    args = _hip.entry_args("masked", "direct", plan=plan, operands=1, out0=2, mask=mask, seeds=None, numel=8, stream=3, out1="ignored", rows="ignored")
    assert args[0]._obj is plan and args[3]._obj is mask and args[1:3] == [1, 2] and args[4:] == [None, 8, 3]
    with pytest.raises(KeyError):
        _hip.entry_args("masked", "direct", plan=plan)


def test_a_step_call_is_the_six_tuple_and_says_its_kind():
    plan, a, b = _hip.StepPlanC(), torch.zeros(8), torch.zeros(8)
    call = _hip.StepCall(plan, (a, b), a, None, None, 8)
    p, inputs, out0, out1, seeds, numel = call
    assert p is plan and inputs == [a, b] and isinstance(inputs, list) and out0 is a and out1 is None and seeds is None and numel == 8
    assert isinstance(call, tuple) and len(call) == 6 and call[:4] == (plan, [a, b], a, None) and call == (plan, [a, b], a, None, None, 8)
    assert [q for q, *_ in [call]] == [plan]
    assert (call.plan, call.inputs, call.out0, call.out1, call.seeds, call.numel) == tuple(call)
    assert call.kind == "plain" and call.layout is None
    assert all(getattr(call, n) is None for n in ("mask", "cond", "guided_out", "scale", "slot", "factor", "phi", "sample_numel"))
    guided = _hip.StepCall(plan, [a, b], a, None, None, 8, "guided_rescaled", cond=b, guided_out=None, scale=7.5, slot=1, factor=a, phi=0.7, sample_numel=4)
    assert len(guided) == 6 and guided.kind == "guided_rescaled" and (guided.cond, guided.scale, guided.slot, guided.factor, guided.phi, guided.sample_numel) == (b, 7.5, 1, a, 0.7, 4)
    masked = _hip.StepCall(plan, [a], a, None, None, 8, "masked", mask=b, mask_numel=8, batch_stride=0, layout=(4, 2))
    assert masked.kind == "masked" and masked.mask is b and masked.layout == (4, 2)
    factor = _hip.FactorCall(a, b, 7.5, 4, a, None)
    assert factor.kind == "guidance_factor" and not isinstance(factor, tuple) and (factor.uncond, factor.cond, factor.scale, factor.sample_numel, factor.factor, factor.stats) == (a, b, 7.5, 4, a, None)
    with pytest.raises(TypeError):
        plan, *_ = factor  # it does not unpack as a plan-led tuple


class StubLib:
    "stands for the library: every launch returns 0 and is remembered by name with its arguments, structures and arrays spelled out"

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith(("skr_step_launch", "skr_guidance_rescale_factor")):
            raise AttributeError(name)

        def launch(*args):
            self.calls.append((name, tuple(spelled(a) for a in args)))
            return 0

        return launch


def spelled(arg):
    if hasattr(arg, "_obj"):  # byref(structure): the structure's fields
        return tuple(getattr(arg._obj, field) for field, _ in arg._obj._fields_ if field != "coef0" and field != "coef1" and field != "convert_k")
    if isinstance(arg, ctypes.Array):
        return list(arg)
    return arg


@pytest.fixture
def lib(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(_hip, "load", lambda: stub)
    monkeypatch.setattr(_hip, "current_stream_ptr", lambda device: STREAM)
    return stub


def test_the_five_launchers_make_the_calls_they_made_before_the_table(lib):
    "what launch_step, launch_step_masked, launch_step_guided, launch_guidance_factor and launch_step_guided_rescaled handed the library before"
    cpu = torch.device("cpu")
    x, o, h, out, out1, cond, stored = (torch.zeros(16, dtype=torch.bfloat16) for _ in range(7))
    mask, factor, seeds, stats = torch.zeros(8, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.float64)
    plan = _hip.StepPlanC()
    plan.n_terms = plan.n_group_a = 3
    plan.dtype_a = plan.out0_dtype = _hip.BF16
    plan.out1_dtype, plan.sample_numel = _hip.NONE, 8
    P = spelled(ctypes.byref(plan))
    arr = [x.data_ptr(), o.data_ptr(), h.data_ptr()]
    _hip.launch_step(plan, [x, o, h], out, out1, seeds, 16, cpu)
    _hip.launch_step(plan, [x, o, h], None, out1, None, 16, cpu, layout=(4, 2))
    _hip.launch_step_masked(plan, [x, o, h], out, mask, 8, 0, seeds, 16, cpu)
    _hip.launch_step_masked(plan, [x, o, h], out, mask, 4, 4, None, 16, cpu, layout=(2, 4))
    _hip.launch_step_guided(plan, [x, o, h], out, cond, stored, 7.5, 1, seeds, 16, cpu)
    _hip.launch_step_guided(plan, [x, o, h], None, cond, None, 2, 0, None, 16, cpu)
    _hip.launch_guidance_factor(o, cond, 7.5, 8, factor, stats)
    _hip.launch_guidance_factor(o, cond, 3, 8, factor)
    _hip.launch_step_guided_rescaled(plan, [x, o, h], out, cond, stored, 7.5, 1, factor, 0.7, 8, seeds, 16, cpu)
    partials = [args[8] for name, args in lib.calls if name == "skr_guidance_rescale_factor"]
    assert len(partials) == 2 and all(isinstance(p, int) and p != 0 for p in partials)  # the workspace is torch's: only its address is new every call
    assert lib.calls == [
        ("skr_step_launch", (P, arr, out.data_ptr(), out1.data_ptr(), seeds.data_ptr(), 16, STREAM)),
        ("skr_step_launch_channels_last", (P, arr, None, out1.data_ptr(), None, (4, 2), 16, STREAM)),
        ("skr_step_launch_masked", (P, arr, out.data_ptr(), (mask.data_ptr(), _hip.BF16, 0, 8, 0), seeds.data_ptr(), 16, STREAM)),
        ("skr_step_launch_masked_channels_last", (P, arr, out.data_ptr(), (mask.data_ptr(), _hip.BF16, 0, 4, 4), None, (2, 4), 16, STREAM)),
        ("skr_step_launch_guided", (P, arr, out.data_ptr(), (cond.data_ptr(), stored.data_ptr(), 7.5, 1, 0), seeds.data_ptr(), 16, STREAM)),
        ("skr_step_launch_guided", (P, arr, None, (cond.data_ptr(), None, 2.0, 0, 0), None, 16, STREAM)),
        ("skr_guidance_rescale_factor", (o.data_ptr(), cond.data_ptr(), _hip.BF16, 7.5, 16, 8, factor.data_ptr(), stats.data_ptr(), partials[0], STREAM)),
        ("skr_guidance_rescale_factor", (o.data_ptr(), cond.data_ptr(), _hip.BF16, 3.0, 16, 8, factor.data_ptr(), None, partials[1], STREAM)),
        ("skr_step_launch_guided_rescaled", (P, arr, out.data_ptr(), (cond.data_ptr(), stored.data_ptr(), 7.5, 1, 0), (factor.data_ptr(), 0.7, 8, 0), seeds.data_ptr(), 16, STREAM)),
    ]
    assert all(type(args[3]) is float for name, args in lib.calls if name == "skr_guidance_rescale_factor")  # float(scale), as ever


def test_the_launchers_trace_records_and_check_under_the_entrys_name(lib, monkeypatch):
    cpu, t = torch.device("cpu"), torch.zeros(16, dtype=torch.bfloat16)
    plan = _hip.StepPlanC()
    _hip.trace = []
    try:
        _hip.launch_step(plan, [t], t, None, None, 16, cpu)
        _hip.launch_step_masked(plan, [t], t, t, 8, 0, None, 16, cpu, layout=(4, 2))
        _hip.launch_step_guided(plan, [t], t, t, None, 7.5, 0, None, 16, cpu)
        _hip.launch_guidance_factor(t, t, 7.5, 8, t)
        _hip.launch_step_guided_rescaled(plan, [t], t, t, None, 7.5, 0, t, 0.7, 8, None, 16, cpu)
        trace = _hip.trace
    finally:
        _hip.trace = None
    assert [e.kind for e in trace] == ["plain", "masked", "guided", "guidance_factor", "guided_rescaled"]
    assert [e.plan for e in trace if e.kind != "guidance_factor"] == [plan] * 4 and trace[0] == (plan, [t], t, None, None, 16)
    assert (trace[1].mask, trace[1].layout, trace[2].scale, trace[2].slot, trace[4].phi, trace[4].sample_numel) == (t, (4, 2), 7.5, 0, 0.7, 8)
    checked = []
    monkeypatch.setattr(_hip, "check", lambda status, what: checked.append(what))
    _hip.launch_step(plan, [t], t, None, None, 16, cpu)
    _hip.launch_step(plan, [t], t, None, None, 16, cpu, layout=(4, 2))
    _hip.launch_step_masked(plan, [t], t, t, 8, 0, None, 16, cpu)
    _hip.launch_step_masked(plan, [t], t, t, 8, 0, None, 16, cpu, layout=(4, 2))
    _hip.launch_step_guided(plan, [t], t, t, None, 7.5, 0, None, 16, cpu)
    _hip.launch_guidance_factor(t, t, 7.5, 8, t)
    _hip.launch_step_guided_rescaled(plan, [t], t, t, None, 7.5, 0, t, 0.7, 8, None, 16, cpu)
    assert checked == ["skr_step_launch", "skr_step_launch_channels_last", "skr_step_launch_masked", "skr_step_launch_masked_channels_last", "skr_step_launch_guided",
                       "skr_guidance_rescale_factor", "skr_step_launch_guided_rescaled"]  # fmt: skip


def test_the_replayed_step_path_builds_no_record_and_makes_one_call(lib, monkeypatch):
    "step_launch_raw without a hook: one getattr on the library, one call -- no StepCall, no table"

    def never(*args, **kwargs):
        raise AssertionError("the hot path touched the record or the table")

    for name in ("StepCall", "entry_name", "entry_args", "call_entry"):
        monkeypatch.setattr(_hip, name, never)
    assert _hip.indexed is None and _hip.trace is None and _hip.hooks_clear()
    plan = _hip.StepPlanC()
    assert _hip.step_launch_raw(plan, None, 1, 2, 3, 16, STREAM) == 0
    assert len(lib.calls) == 1 and lib.calls[0][0] == "skr_step_launch" and lib.calls[0][1][1:] == (None, 1, 2, 3, 16, STREAM)
