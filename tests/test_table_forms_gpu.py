"""The table forms of the one-trip step kernels (needs an MI355X): skr_step_launch_indexed, skr_step_launch_indexed_per_sample and
skr_step_launch_rolling at every operand count, dtype and form csrc/skr_step_fast.hip instantiates (tests/table_cases.py holds the grid).

include/skrample_hip.h promises that a sample's result in any table form has the bits of the narrower skr_step_launch that holds exactly
the present operands in slot order, so the main assertion has no tolerance.  What the kernarg and table forms could get wrong TOGETHER is
held to a float64 evaluation on the host (bound: table_cases.reference64; measured margins: profiles/table_forms_margins.txt)."""

import ctypes

import pytest
import table_cases as TC
import torch
from conftest import note_margin

from skrample_amd import _hip

pytestmark = pytest.mark.gpu

PATTERN16, PATTERN32 = 0x4A5B, 0x4A5B4A5B
IDS = [(family, form, dtype) for family in ("k1", "rk1", "k2") for form in TC.FORMS for dtype in TC.FAMILY_DTYPES[family]]


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def sentinel(td: torch.dtype, n: int, dev) -> torch.Tensor:
    "n elements behind and in front of a guard, all of them a fixed bit pattern"
    buf = torch.empty(n + 2 * TC.GUARD, dtype=td, device=dev)
    int_view(buf).fill_(PATTERN16 if buf.element_size() == 2 else PATTERN32)
    return buf


def pattern_of(t: torch.Tensor) -> int:
    return PATTERN16 if t.element_size() == 2 else PATTERN32


_device_pools: dict = {}


def device_pool(dtype: str, batch: int, sample: int, dev):
    key = (dtype, batch, sample)
    if key not in _device_pools:
        narrow, wide = TC.pool(dtype, batch, sample)
        _device_pools[key] = (narrow.to(dev), wide.to(dev), TC.seeds_tensor(TC.seeds_for(batch)).to(dev))
    return _device_pools[key]


class Runner:
    "one (case, dtype, geometry): the operands, the table on the device, and the launches of both sides of a comparison"

    def __init__(self, lib, dev, case: TC.Case, dtype: str, geometry, rolling: bool):
        self.lib, self.dev, self.case, self.dtype, self.td = lib, dev, case, dtype, TC.DTYPES[dtype]
        self.batch, self.sample = geometry
        self.n = self.batch * self.sample
        self.narrow, self.wide, self.seeds_dev = device_pool(dtype, self.batch, self.sample, dev)
        self.seeds = TC.seeds_for(self.batch)
        self.rows, self.present = TC.build_rows(case, rolling)
        self.rows_dev = TC.rows_tensor(self.rows).to(dev)
        self.plan = TC.make_plan(case, _hip.DTYPE_CODE[self.td], self.sample)
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.out_dtypes = {"k1": (self.td, None), "rk1": (self.td, self.td), "k2": (torch.float32, self.td)}[case.family]

    def outputs(self):
        return [sentinel(od, self.n, self.dev) if od is not None else None for od in self.out_dtypes]

    @staticmethod
    def body_ptr(buf, at: int = 0):
        return None if buf is None else buf.data_ptr() + (TC.GUARD + at) * buf.element_size()

    def operands(self, picks, off):
        "the operand tensors of one launch: for a rolling launch a copy in which every absent operand of a sample, and every operand of an inactive one, is NaN"
        narrow, wide = self.narrow, self.wide
        if any(p < 0 for p in picks) or any(len(self.present[p + off]) < self.case.slots for p in picks if p >= 0):
            narrow, wide = narrow.clone(), wide.clone()
            for b, p in enumerate(picks):
                part = slice(b * self.sample, (b + 1) * self.sample)
                gone = range(self.case.slots) if p < 0 else [j for j in range(self.case.slots) if j not in self.present[p + off]]
                for j in gone:
                    (narrow[j] if j < self.case.na else wide)[part] = float("nan")
        return narrow, wide

    def pointers(self, narrow, wide, slots, at: int = 0):
        ptrs = [narrow[j].data_ptr() + at * narrow.element_size() if j < self.case.na else wide.data_ptr() + at * 4 for j in slots]
        return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)

    def table_launch(self, form, picks, off, narrow=None, wide=None):
        "one table launch into fresh sentinel outputs: (out0 buffer, out1 buffer); the index tensor stays alive until the caller synchronises"
        narrow, wide = (self.narrow, self.wide) if narrow is None else (narrow, wide)
        o0, o1 = self.outputs()
        self.index = torch.tensor(picks, dtype=torch.int32, device=self.dev)
        fn = {"whole": self.lib.skr_step_launch_indexed, "per_sample": self.lib.skr_step_launch_indexed_per_sample, "rolling": self.lib.skr_step_launch_rolling}[form]
        seeds = self.seeds_dev.data_ptr() if self.case.draws else None
        rc = fn(ctypes.byref(self.plan), self.pointers(narrow, wide, range(self.case.slots)), self.body_ptr(o0), self.body_ptr(o1), seeds, self.n,
                self.rows_dev.data_ptr(), self.index.data_ptr(), off, self.stream)  # fmt: skip
        assert rc == 0, (self.case, form, picks, off, rc)
        return o0, o1

    def narrow_launches(self, sample_rows, narrow, wide):
        "the yardstick: one skr_step_launch per active sample on its own slices, present operands only, into sentinel outputs"
        o0, o1 = self.outputs()
        for b, r in enumerate(sample_rows):
            if r is None:
                continue
            at = b * self.sample
            one = TC.narrow_plan(self.case, self.plan, self.rows[r], self.present[r])
            seeds = self.seeds_dev[b : b + 1].data_ptr() if self.case.draws else None
            rc = self.lib.skr_step_launch(ctypes.byref(one), self.pointers(narrow, wide, self.present[r], at), self.body_ptr(o0, at), self.body_ptr(o1, at), seeds, self.sample, self.stream)
            assert rc == 0, (self.case, b, r, rc)
        return o0, o1

    def sample_rows(self, form, picks, off):
        if form == "whole":
            return [picks[0] + off] * self.batch
        return [p + off if p >= 0 else None for p in picks]


def check_case(run: Runner, form: str, picks, off: int, worst: dict, float64: bool = True):
    "assertions 1-3 of one launch: bits against the narrow launches, float64 bound, untouched bytes"
    case, S = run.case, run.sample
    narrow, wide = run.operands(picks, off) if form == "rolling" else (run.narrow, run.wide)
    got = run.table_launch(form, picks, off, narrow, wide)
    rows_of = run.sample_rows(form, picks, off)
    want = run.narrow_launches(rows_of, narrow, wide)
    torch.cuda.synchronize()
    what = (case, run.dtype, form, (run.batch, S), picks, off)
    x64 = TC.operands64(case, run.dtype, run.batch, S) if float64 else None
    host = {}
    for name, g, w in zip(("out0", "out1"), got, want):
        if g is None:
            continue
        gc = g.cpu()
        gi, wi = int_view(gc), int_view(w).cpu()
        pat = pattern_of(g)
        assert (gi[: TC.GUARD] == pat).all() and (gi[TC.GUARD + run.n :] == pat).all(), ("guard overwritten", name, what)
        for b, r in enumerate(rows_of):
            part = slice(TC.GUARD + b * S, TC.GUARD + (b + 1) * S)
            if r is None:
                assert (gi[part] == pat).all(), ("inactive sample written", name, b, what)
                continue
            assert torch.equal(gi[part], wi[part]), ("bits differ from the narrow launch", name, b, r, int((gi[part] != wi[part]).sum()), what)
            assert not torch.isnan(gc[part].float()).any(), ("NaN in an active sample", name, b, r, what)
        host[name] = gc[TC.GUARD : TC.GUARD + run.n].view(run.batch, S)
    if not float64:
        return got
    for b, r in enumerate(rows_of):
        if r is None:
            continue
        row, present = run.rows[r], run.present[r]
        conv = None
        if case.family == "rk1":
            cpu_narrow = TC.pool(run.dtype, run.batch, S)[0]
            s_, o_ = (cpu_narrow[j, b * S : (b + 1) * S] for j in (0, 1))
            conv = TC.conversion_reference(s_, o_, case.kinds, tuple(row.convert_k))
            assert torch.equal(int_view(host["out0"][b]), int_view(conv)), ("rounded conversion differs from torch op by op", b, r, what)
        for name, (ref, allowed) in TC.reference64(case, run.td, x64[:, b, :], row, present, run.seeds[b], conv).items():
            ratio = TC.worst_ratio(host[name][b], ref, allowed)
            key = f"{case.family}/{run.dtype}/{name}"
            worst[key] = max(worst.get(key, 0.0), ratio)
            assert ratio <= 1.0, ("float64 bound", name, b, r, ratio, what)
    return got


def forced_block(lib, case):
    if case.family == "rk1":
        assert lib.skr_set_tuning(b"rk_blk", case.blk) == 0


@pytest.mark.parametrize(("family", "form", "dtype"), IDS, ids=["-".join(i) for i in IDS])
def test_every_count_matches_the_narrow_launch_and_float64(family, form, dtype, dev):
    """Every instantiated operand count of one kernel family in one table form and dtype, on 4 samples of 1, 2 and 3 chunks with row_offset 0
    and 1: per sample the bits of the narrow skr_step_launch, the float64 bound, sentinel bytes kept by inactive samples and guards."""
    lib = _hip.load()
    worst: dict = {}
    try:
        for n_case, case in enumerate(TC.full_grid(family)):
            forced_block(lib, case)
            for geometry, off in TC.SMALL_COMBOS:
                run = Runner(lib, dev, case, dtype, geometry, rolling=form == "rolling")
                for picks in TC.pick_lists(form, len(run.rows), run.batch, off, n_case):
                    check_case(run, form, picks, off, worst)
    finally:
        lib.skr_set_tuning(b"reset", 0)
    for key, ratio in worst.items():
        note_margin("table_forms", f"{key}/{form} err/allowed", ratio, 1.0)
        print(f"table_forms {key}/{form}: worst err/allowed {ratio:.4f}")
    assert worst


MAPPED_IDS = [(family, dtype) for family in ("k1", "rk1", "k2") for dtype in TC.FAMILY_DTYPES[family]]


@pytest.mark.parametrize(("family", "dtype"), MAPPED_IDS, ids=["-".join(i) for i in MAPPED_IDS])
def test_row_selection_under_the_xcd_chunk_map(family, dtype, dev):
    """64 samples of 3 chunks (192 chunks: the XCD chunk map keeps a non-zero run length, and the chunk -> sample map divides) with shuffled
    per-sample rows, in the per-sample and the rolling form: the same three assertions, and the identity chunk map gives the same bits."""
    lib = _hip.load()
    worst: dict = {}
    try:
        for n_case, case in enumerate(TC.mapped_grid(family)):
            for form in ("per_sample", "rolling"):
                lib.skr_set_tuning(b"reset", 0)
                forced_block(lib, case)
                run = Runner(lib, dev, case, dtype, TC.MAPPED, rolling=form == "rolling")
                off = n_case % 2
                picks = TC.pick_lists(form, len(run.rows), run.batch, off, 100 + n_case)[0]
                got = check_case(run, form, picks, off, worst)
                assert lib.skr_set_tuning(b"xmap", 0) == 0
                narrow, wide = run.operands(picks, off) if form == "rolling" else (run.narrow, run.wide)
                identity = run.table_launch(form, picks, off, narrow, wide)
                torch.cuda.synchronize()
                for g, i in zip(got, identity):
                    assert g is None or torch.equal(int_view(g), int_view(i)), ("identity chunk map differs", case, form, dtype)
    finally:
        lib.skr_set_tuning(b"reset", 0)
    for key, ratio in worst.items():
        note_margin("table_forms", f"{key}/mapped err/allowed", ratio, 1.0)
        print(f"table_forms {key}/mapped: worst err/allowed {ratio:.4f}")
    assert worst


@pytest.mark.parametrize(("family", "dtype"), MAPPED_IDS, ids=["-".join(i) for i in MAPPED_IDS])
def test_the_three_forms_agree(family, dtype, dev):
    """A per-sample launch whose index vector is constant equals the whole-batch launch with that index; a rolling launch with every sample
    active and no absent operand equals the per-sample launch with the same vector.  Every count, 4 samples of 3 chunks."""
    lib = _hip.load()
    try:
        for n_case, case in enumerate(TC.full_grid(family)):
            forced_block(lib, case)
            run = Runner(lib, dev, case, dtype, TC.SMALL[2], rolling=False)
            off = n_case % 2
            r = n_case % (TC.N_DENSE - off)
            mixed = [(n_case + 2 * b) % (TC.N_DENSE - off) for b in range(run.batch)]
            whole = run.table_launch("whole", [r], off)
            constant = run.table_launch("per_sample", [r] * run.batch, off)
            per_sample = run.table_launch("per_sample", mixed, off)
            rolling = run.table_launch("rolling", mixed, off)
            torch.cuda.synchronize()
            for a, b, c, d in zip(whole, constant, per_sample, rolling):
                if a is None:
                    continue
                assert torch.equal(int_view(a), int_view(b)), ("constant per-sample index differs from the whole-batch launch", case, dtype, r, off)
                assert torch.equal(int_view(c), int_view(d)), ("rolling launch differs from the per-sample launch", case, dtype, mixed, off)
                assert not torch.equal(int_view(a), int_view(c))  # (the rows do differ)
    finally:
        lib.skr_set_tuning(b"reset", 0)


def test_requests_outside_the_table_forms_are_refused(dev):
    "SKR_ERR_UNSUPPORTED, nothing written: 17 operands, a two-output count without an instantiation, two outputs of fp32 operands, fp64 accumulation, a negative row_offset"
    lib = _hip.load()
    batch, sample = TC.SMALL[0]
    n = batch * sample
    narrow, wide, seeds = device_pool("bf16", batch, sample, dev)
    narrow32, _, _ = device_pool("fp32", batch, sample, dev)
    extra = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    rows, _ = TC.build_rows(TC.Case("k1", 16, noise="on"), rolling=False)
    rows_dev = TC.rows_tensor(rows).to(dev)
    index = torch.ones(batch, dtype=torch.int32, device=dev)  # with row_offset 0 and -1 alike every entry names a row of the table
    stream = torch.cuda.current_stream(dev).cuda_stream
    launches = {"whole": lib.skr_step_launch_indexed, "per_sample": lib.skr_step_launch_indexed_per_sample, "rolling": lib.skr_step_launch_rolling}

    def refused(case, code, tensors, off=0, acc_f64=0, out_dtypes=None):
        plan = TC.make_plan(case, code, sample)
        plan.acc_f64 = acc_f64
        if out_dtypes is not None:
            plan.out0_dtype, plan.out1_dtype = (_hip.DTYPE_CODE[d] for d in out_dtypes)
        outs = [sentinel(_hip.CODE_DTYPE[c], n, dev) if c != _hip.NONE else None for c in (plan.out0_dtype, plan.out1_dtype)]
        ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        for form, fn in launches.items():
            rc = fn(ctypes.byref(plan), ptrs, Runner.body_ptr(outs[0]), Runner.body_ptr(outs[1]), seeds.data_ptr(), n, rows_dev.data_ptr(), index.data_ptr(), off, stream)
            torch.cuda.synchronize()
            assert rc == _hip.SKR_ERR_UNSUPPORTED, (case, form, rc)
        for o in outs:
            assert o is None or (int_view(o) == pattern_of(o)).all(), case

    bf16, f32 = _hip.BF16, _hip.F32
    refused(TC.Case("k1", 17, noise="on"), bf16, list(narrow) + [extra])
    refused(TC.Case("k1", 17), bf16, list(narrow) + [extra])
    refused(TC.Case("k2", 5, 1, noise="both"), bf16, list(narrow[:5]) + [wide])
    refused(TC.Case("k2", 4, 0), f32, list(narrow32[:4]), out_dtypes=(torch.float32, torch.float32))
    refused(TC.Case("k1", 4, noise="on"), bf16, list(narrow[:4]), acc_f64=1)
    refused(TC.Case("k2", 4, 1), bf16, list(narrow[:4]) + [wide], acc_f64=1)
    refused(TC.Case("k1", 4, noise="on"), bf16, list(narrow[:4]), off=-1)
    refused(TC.Case("rk1", 4, kinds=(1, 2)), bf16, list(narrow[:4]), off=-1)
